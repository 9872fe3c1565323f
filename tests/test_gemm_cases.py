"""CPU checks of tests/gemm_cases.py: every case sits in the launch regime it is labelled with, the cases together reach every regime
of csrc/gemm.hip, the mirror's workspace and table arithmetic equals the built library's, torch's float32 CPU product alone meets the
derived bound the GPU test applies (no case is born failing), a dropped k term misses it a hundredfold, and four emulated kernel
faults are caught by the comparison the GPU test uses."""
import ctypes

import pytest
import torch

import gemm_cases as gc

ALL = list(gc.CASES)


def _in_regime(launch, regime):
    for k, v in regime.items():
        assert launch[k] == v, (k, launch[k], v, launch)


@pytest.mark.parametrize('name', ALL)
def test_case_reaches_its_regime(name):
    case = gc.CASES[name]
    assert case['regime'], 'a case without a label'
    _in_regime(gc.case_regime(case), case['regime'])


@pytest.mark.parametrize('name', list(gc.TABLES))
def test_table_reaches_its_layout(name):
    orient, entries, layout = gc.TABLES[name]
    regs = [gc.case_regime(e, table=True) for e in gc.table_entries(name)]
    assert all(r['orient'] == gc.ORIENTS[orient] and r['store'] == 'atomic' and not r['zero_fill'] for r in regs)
    _in_regime(gc.table_layout(regs), layout)
    for e in entries:                                                # a shared destination is the same view
        assert e['share'] is None or (entries[e['share']]['shape'][:2], entries[e['share']]['dest']) == (e['shape'][:2], e['dest'])


def test_case_table_covers_the_regimes():
    regs = {n: gc.case_regime(c) for n, c in gc.CASES.items()}
    R = list(regs.values())

    def have(**kv):
        return any(all(r[k] == v for k, v in kv.items()) for r in R)
    for o in gc.ORIENTS.values():                                    # every orientation with 16-byte and with scalar loads on both operands
        assert have(orient=o, a_vec=True, b_vec=True) and have(orient=o, a_vec=False, b_vec=False), o
    for op in ('a_tail', 'b_tail'):                                  # both scalar-tail kinds, and a 16-byte load without one
        assert {r[op] for r in R} == {None, 'k', 'row'}
    assert have(a_vec=True, a_tail=None) and have(b_vec=True, b_tail=None)
    assert {r['store'] for r in R} == {'vec', 'scalar', 'atomic'}
    for st in ('vec', 'scalar', 'atomic'):
        assert have(store=st, partial_quad=True) and have(store=st, partial_quad=False), st
    assert {r['mode'] for r in R} == {'single', 'atomic', 'parked'}
    assert have(zero_fill=True) and have(mode='atomic', zero_fill=False) and have(fold=True) and have(fold=False)
    assert {r['fold_groups'] for r in R} == {0, 1, 2}
    assert any(r['empty_slices'] > 0 and r['mode'] == m for r in R for m in ('parked',)) and have(mode='atomic', empty_slices=1)
    assert have(one_tile_slice=True, prefetch=False) and have(prefetch=True)
    assert any(r['live_slices'] > 1 and r['slices'][r['live_slices'] - 1][1] % gc.GBK for r in R), 'a ragged last slice'
    assert have(partial=(False, False)) and have(partial=(True, True)) and any(max(r['tiles']) > 2 for r in R)
    assert have(rowsum_idle_columns=True, mode='single') and have(rowsum_idle_columns=True, mode='atomic') \
        and have(rowsum_idle_columns=True, mode='parked')
    assert have(bias_once=True)
    assert any(r['grid'][2] > r['live_slices'] + r['empty_slices'] for r in R), 'batch > 1'
    assert {(r['big'][2], r['big'][3]) for r in R} == {(None, None), ('128x128', '128x64')}
    assert all(r['big'][0] is None for r in R)
    # the big-tile cases: M of 128 and of 130, N partial against 128 and against 64
    big = [gc.CASES[n]['shape'] for n in gc.BIG_CASES]
    assert {s[0] for s in big} == {128, 130} and all(s[1] % 128 and s[1] % 64 and s[2] % gc.GBK for s in big)
    # the tables: all four orientation codes, parked / unparked / parked, an unparked first entry, the special entries
    codes = set()
    for name, (_, entries, layout) in gc.TABLES.items():
        codes.add(layout['code'])
    assert codes == {0, 1, 2, 3}
    modes = {name: [e['mode'] for e in es] for name, (_, es, _) in gc.TABLES.items()}
    for code in range(4):
        assert any(layout['code'] == code and [m == 'parked' for m in modes[name][:3]] == [True, False, True]
                   for name, (_, _, layout) in gc.TABLES.items()), code
    every = [e for _, es, _ in gc.TABLES.values() for e in es]
    assert any(m[0] != 'parked' for m in modes.values()) and any(e['share'] is not None for e in every) and any(e['rowsum'] for e in every)
    assert any(e['batch'] > 1 for e in every) and any(e['mode'] == 'atomic' for e in every)
    # the shapes the older tests run stay on the easy path -- which is why this table exists
    r0 = gc.gemm_regime(37, 88, 64, 64, 1, 1, 64, 88, 1)
    assert r0['orient'] == (True, True) and r0['a_tail'] is None and r0['store'] == 'vec' and r0['mode'] == 'single'


def test_tie_rule_and_kper_by_hand():
    """values worked out from csrc/gemm.hip by hand, so that an edit of the mirror itself shows"""
    assert gc.gemm_regime(4, 4, 4, 1, 1, 1, 1, 4, 1)['orient'] == (True, True)           # sak == sam, sbk == sbn: k-fast
    assert gc.gemm_regime(4, 4, 4, 1, 2, 2, 1, 4, 1)['orient'] == (False, False)
    assert gc.kslices(229, 3) == (96, [(0, 96), (96, 192), (192, 229)])
    assert gc.kslices(33, 3) == (32, [(0, 32), (32, 33), (64, 33)])
    assert gc.kslices(300, 4) == (96, [(0, 96), (96, 192), (192, 288), (288, 300)])
    assert gc.workspace_bytes(70, 88, 3, 1) == 3 * 4 * 16384 + 3 * 70 * 4 and gc.workspace_bytes(70, 88, 1, 1) == 0
    r = gc.gemm_regime(70, 88, 229, 229, 1, 1, 229, 88, 1, splitk=3, parked=True, a_rowsum=True)
    assert r['rs_offset'] == 3 * 4 * 4096 and r['fold_groups'] == 1 and r['a_tail'] == 'k' and r['ktiles'] == [3, 3, 2]


@pytest.fixture(scope='module')
def built():
    from reconvat_amd import build
    return ctypes.CDLL(build.build())


def test_workspace_formula_equals_the_library(built):
    fn = built.rv_gemm_splitk_workspace_bytes
    fn.restype = ctypes.c_long
    for M, N in ((1, 1), (64, 64), (65, 67), (130, 229), (70, 88)):
        for sk in (1, 2, 3, 8):
            for batch in (1, 3):
                assert fn(M, N, sk, batch) == gc.workspace_bytes(M, N, sk, batch), (M, N, sk, batch)


@pytest.mark.parametrize('name', list(gc.TABLES))
def test_table_layout_equals_the_library(built, name):
    """rv_gemm_table_fill / rv_gemm_table_finalize are host arithmetic on host memory: run them on made-up (never dereferenced) pointers
    and read block0, gx, gy, fold0 -- the last four ints of an entry -- back"""
    I, L, P = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    built.rv_gemm_table_entry_bytes.restype = L
    built.rv_gemm_table_fill.restype = L
    built.rv_gemm_table_fill.argtypes = [P, P, L, L, P, L, L, P, L, L, P, I, I, I, I, I, L, L, L, P, P]
    built.rv_gemm_table_finalize.restype = L
    built.rv_gemm_table_finalize.argtypes = [P, I, P]
    nbytes = built.rv_gemm_table_entry_bytes()
    entries = gc.table_entries(name)
    host = torch.zeros(len(entries) * nbytes, dtype=torch.uint8)
    regs = []
    for i, e in enumerate(entries):
        ar, (M, N, K) = gc.case_args(e), e['shape']
        code = built.rv_gemm_table_fill(host.data_ptr() + i * nbytes, 4096, ar['A'][1], ar['A'][2], 4096, ar['B'][1], ar['B'][2], 4096, ar['C'][1],
                                        ar['C'][2], None, M, N, K, e['splitk'], e['batch'], ar['A'][3], ar['B'][3], ar['C'][3], None,
                                        4096 if e['mode'] == 'parked' else None)
        regs.append(gc.case_regime(e, table=True))
        assert code == gc.table_layout(regs[-1:])['code']
    fold = ctypes.c_long(-1)
    total = built.rv_gemm_table_finalize(host.data_ptr(), len(entries), ctypes.addressof(fold))
    want = gc.table_layout(regs)
    tail = host.view(len(entries), nbytes)[:, nbytes - 16:].contiguous().view(torch.int32)
    assert (total, fold.value) == (want['blocks'], want['fold_blocks'])
    assert tail[:, 0].tolist() == want['block0'] and tail[:, 3].tolist() == want['fold0']
    assert [(int(t[1]), int(t[2])) for t in tail] == [r['grid'][:2] for r in regs]


# the per-case checks below run group by group (the first word of a case's name; the shape cases: one group per shape)
GROUPS = {}
for _n in ALL:
    GROUPS.setdefault(' '.join(_n.split()[:2]) if _n.startswith('shape') else _n.split()[0], []).append(_n)


@pytest.mark.parametrize('group', list(GROUPS))
def test_float32_reference_meets_the_bound(group):
    """torch's float32 CPU product, as one `a @ b` and as the mirror's slices summed in k order, under the comparison of the GPU test"""
    for name in GROUPS[group]:
        pr = gc.problem(gc.CASES[name], 'float')
        for order in ('plain', 'slices'):
            c, c2, rs = gc.emulate(pr, order=order)
            for key, ratio in gc.compare(pr, c, c2, rs).items():
                gc.check('cpu-f32 ' + order, name, key, ratio)


@pytest.mark.parametrize('group', list(GROUPS))
def test_integer_problem_is_exact_in_float32(group):
    for name in GROUPS[group]:
        pr = gc.problem(gc.CASES[name], 'int')
        ref = gc.reference(pr)
        for t in (pr['A'], pr['B'], pr['bias'], pr['C0'], pr['rs0']):
            assert t is None or bool(((t.abs() >= 1) & (t.abs() <= 3) & (t == t.round())).all().item())
        assert ref['pre'].abs().max().item() < 2 ** 24
        got = pr['A'] @ pr['B']
        if pr['case']['bias']:
            got = got + pr['bias']
        assert torch.equal(got.double(), ref['pre']), name
        for order in ('plain', 'slices'):
            c, c2, rs = gc.emulate(pr, order=order)
            for key, ratio in gc.compare(pr, c, c2, rs).items():
                gc.check('cpu-int ' + order, name, key, ratio)
                assert pr['case']['act'] or ratio == 0.0, name


@pytest.mark.parametrize('group', list(GROUPS))
def test_a_dropped_k_term_misses_the_bound_a_hundredfold(group):
    """the float problem: every element of the pre-activation moves by >= 100 bounds when the last k term is left out"""
    for name in GROUPS[group]:
        pr = gc.problem(gc.CASES[name], 'float')
        ref, cut = gc.reference(pr), gc.reference(pr, k_drop=1)
        assert ((cut['pre'] - ref['pre']).abs() / ref['bound_pre']).min().item() >= 100, name


@pytest.mark.parametrize('kind', ['int', 'float'])
@pytest.mark.parametrize('group', list(GROUPS))
def test_emulated_faults_are_caught(group, kind):
    """the last k column dropped, the last row never stored, a slice skipped, the row sum added once per n-tile"""
    for name in GROUPS[group]:
        case = gc.CASES[name]
        pr = gc.problem(case, kind)
        reg = gc.case_regime(case)
        faults = ['drop_k', 'drop_row'] + (['skip_slice'] if reg['live_slices'] > 1 else []) + (['rowsum_per_ntile'] if reg['rowsum_idle_columns'] else [])
        for fault in faults:
            c, c2, rs = gc.emulate(pr, fault=fault)
            ratios = gc.compare(pr, c, c2, rs)
            key = 'rs' if fault == 'rowsum_per_ntile' else 'c'
            assert ratios[key] > 1.0, (name, kind, fault, ratios)
            if case['c2'] and fault != 'rowsum_per_ntile':
                assert ratios['c2'] > 1.0, (name, kind, fault, ratios)
