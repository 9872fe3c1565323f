"""The linear GEMM of csrc/gemm.hip through the C ABI at every launch regime of tests/gemm_cases.py: the integer problem against the
int64 product with `==`, the float problem against float64 under the derived per-element bound, operands in NaN-padded buffers,
destinations in buffers whose padding must come back bit-unchanged, NaN-filled split-K workspaces; the bit identities the kernel
documents (parked split-K repeats and equals the in-order sum of its slices, a table entry equals the direct call, the big tiles
equal the 64 x 64 kernel) and the argument refusals.  Every measured ratio error / bound is appended to gemm_errors.jsonl, next to
the parity_errors.jsonl of tests/parity_tol.py."""
import ctypes

import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

NAN = float('nan')
ALL = list(gc.CASES)
PARKED = [n for n in ALL if gc.CASES[n]['mode'] == 'parked']
PARKED_PLAIN = [n for n in PARKED if not (gc.CASES[n]['bias'] or gc.CASES[n]['act'] or gc.CASES[n]['acc'] or gc.CASES[n]['c2'])]


def _lib():
    from reconvat_amd import _lib
    return _lib


def _bits(t):
    return t.detach().cpu().view(torch.int32)


def upload(dev, pr, zero=False):
    """fresh device copies of the problem's buffers (zero: the live regions of the destinations start at 0)"""
    d = {k: pr[k + '_buf'].to(dev) if k + '_buf' in pr else None for k in ('A', 'B', 'bias', 'C', 'C2', 'rs')}
    if zero:
        gc.live(pr, 'C', d['C']).zero_()
        if d['rs'] is not None:
            d['rs'][1:1 + pr['case']['shape'][0]] = 0.0
    return d


def _at(t, off):
    return None if t is None else t.data_ptr() + 4 * off


def workspace(dev, pr, splitk, parked):
    """NaN-filled: the ABI calls it uninitialised"""
    if not (parked and splitk > 1):
        return None
    M, N, _ = pr['case']['shape']
    nbytes = _lib().load().rv_gemm_splitk_workspace_bytes(M, N, splitk, pr['case']['batch'])
    assert nbytes == gc.workspace_bytes(M, N, splitk, pr['case']['batch'])
    return torch.full((nbytes // 4,), NAN, device=dev)


def gemm_args(pr, d, ws, splitk=None, acc=None, kslice=None):
    """the arguments of rv_gemm for the problem on the buffers `d` (kslice = (k0, k1): the sub-view of A and B over that k range)"""
    case, ar = pr['case'], pr['args']
    M, N, K = case['shape']
    (oa, sam, sak, bsa), (ob, sbk, sbn, bsb), (oc, scm, scn, bsc) = ar['A'], ar['B'], ar['C']
    if kslice is not None:
        oa, ob, K = oa + kslice[0] * sak, ob + kslice[0] * sbk, kslice[1] - kslice[0]
    o2, s2m, s2n, _ = ar['C2'] if case['c2'] else (0, 0, 0, 0)
    return (_at(d['A'], oa), sam, sak, _at(d['B'], ob), sbk, sbn, _at(d['C'], oc), scm, scn, _at(d['C2'], o2), s2m, s2n, _at(d['bias'], 0),
            M, N, K, case['act'], case['acc'] if acc is None else acc, case['splitk'] if splitk is None else splitk, case['batch'],
            bsa, bsb, bsc, _at(d['rs'], 1), None if ws is None else ws.data_ptr(), None, _lib().stream())


def collect(pr, d):
    """after the launches: inputs untouched, paddings intact -> (c [batch, M, N], c2, rs) on the CPU"""
    torch.cuda.synchronize()
    for k in ('A', 'B', 'bias'):
        assert d[k] is None or torch.equal(_bits(d[k]), pr[k + '_buf'].view(torch.int32)), 'the GEMM wrote into ' + k
    c_buf = d['C'].cpu()
    assert gc.padding_intact(pr, 'C', c_buf), 'the GEMM wrote into the padding of C'
    c2 = rs = None
    if d['C2'] is not None:
        c2_buf = d['C2'].cpu()
        assert gc.padding_intact(pr, 'C2', c2_buf), 'the GEMM wrote into the padding of C2'
        c2 = gc.live(pr, 'C2', c2_buf).clone()
    if d['rs'] is not None:
        rs_buf = d['rs'].cpu()
        assert gc.padding_intact(pr, 'rs', rs_buf), 'the GEMM wrote into the padding of a_rowsum'
        rs = rs_buf[1:1 + pr['case']['shape'][0]].clone()
    return gc.live(pr, 'C', c_buf).clone(), c2, rs


def run(dev, pr, zero=False, acc=None):
    d = upload(dev, pr, zero)
    ws = workspace(dev, pr, pr['case']['splitk'], pr['case']['mode'] == 'parked')
    _lib().call('rv_gemm', *gemm_args(pr, d, ws, acc=acc))
    return collect(pr, d)


def same_bits(a, b):
    return a is b or torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# every case, both problems
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['int', 'float'])
@pytest.mark.parametrize('name', ALL)
def test_gemm_case(dev, name, kind):
    pr = gc.problem(gc.CASES[name], kind)
    c, c2, rs = run(dev, pr)
    ratios = gc.compare(pr, c, c2, rs)
    print(name, kind, ratios)
    for key, ratio in ratios.items():
        gc.check('rv_gemm ' + kind, name, key, ratio, log=True)


# ---------------------------------------------------------------------------------------------------------------------
# bit identities (the float problem)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PARKED)
def test_parked_splitk_repeats_bit_for_bit(dev, name):
    pr = gc.problem(gc.CASES[name], 'float')
    first, second = run(dev, pr), run(dev, pr)
    assert all(same_bits(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize('name', PARKED_PLAIN)
def test_parked_splitk_is_the_in_order_sum_of_its_slices(dev, name):
    """each k slice of the mirror as a splitk = 1 call on the sub-views of A and B, added in k order in float32: pins kper and the order
    of the fold"""
    case = gc.CASES[name]
    pr = gc.problem(case, 'float')
    parked, _, _ = run(dev, pr)
    _, slices = gc.kslices(case['shape'][2], case['splitk'])
    total = None
    for k0, k1 in slices:
        if k0 >= k1:
            continue                                                 # an empty slice parks zeros
        d = upload(dev, pr)
        _lib().call('rv_gemm', *gemm_args(pr, d, None, splitk=1, kslice=(k0, k1)))
        part, _, _ = collect(pr, d)
        total = part if total is None else total + part
    assert torch.equal(parked, total)


@pytest.mark.parametrize('policy', [2, 3])
@pytest.mark.parametrize('kind', ['int', 'float'])
@pytest.mark.parametrize('name', gc.BIG_CASES)
def test_big_tiles_equal_the_64x64_kernel(dev, name, kind, policy):
    case = gc.CASES[name]
    assert gc.case_regime(case)['big'][policy] == {2: '128x128', 3: '128x64'}[policy]
    pr = gc.problem(case, kind)
    setmode = _lib().load().rv_debug_set_gemm_big
    prev = setmode(0)
    try:
        base, _, _ = run(dev, pr)
        setmode(policy)
        big, _, _ = run(dev, pr)
    finally:
        setmode(prev)
    assert same_bits(big, base)
    gc.check('rv_gemm big policy %d %s' % (policy, kind), name, 'c', gc.compare(pr, big)['c'], log=True)


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
def run_table(dev, name, kind, zero=False):
    """-> per entry (problem, device buffers); entries with `share` use the destination buffer of the entry they name"""
    lib = _lib()
    entries = gc.table_entries(name)
    nbytes = lib.load().rv_gemm_table_entry_bytes()
    host = torch.zeros(len(entries) * nbytes, dtype=torch.uint8)
    prs, ds, keep, regs = [], [], [], []
    for i, e in enumerate(entries):
        pr = gc.problem(e, kind)
        d = upload(dev, pr, zero)
        if e['share'] is not None:
            assert entries[e['share']]['shape'][:2] == e['shape'][:2] and entries[e['share']]['dest'] == e['dest']
            d['C'] = ds[e['share']]['C']
        ws = workspace(dev, pr, e['splitk'], e['mode'] == 'parked')
        a = gemm_args(pr, d, ws)
        code = lib.invoke('rv_gemm_table_fill', host.data_ptr() + i * nbytes, *a[:9], a[12], *a[13:16], a[18], a[19], *a[20:23], a[23], a[24])
        regs.append(gc.case_regime(e, table=True))
        assert code == gc.table_layout(regs[-1:])['code'], lib.last_error()
        prs.append(pr)
        ds.append(d)
        keep.append(ws)
    fold = ctypes.c_long(-1)
    total = lib.invoke('rv_gemm_table_finalize', host.data_ptr(), len(entries), ctypes.addressof(fold))
    want = gc.table_layout(regs)
    assert (total, fold.value, want['code']) == (want['blocks'], want['fold_blocks'], gc.TABLES[name][2]['code'])
    table = host.to(dev)
    lib.call('rv_gemm_table_run', table.data_ptr(), len(entries), total, fold.value, want['code'], lib.stream())
    torch.cuda.synchronize()
    return entries, prs, ds


@pytest.mark.parametrize('kind', ['int', 'float'])
@pytest.mark.parametrize('name', list(gc.TABLES))
def test_gemm_table(dev, name, kind):
    entries, prs, ds = run_table(dev, name, kind)
    sharers = {i: [j for j, e in enumerate(entries) if e['share'] == i] for i in range(len(entries))}
    for i, (e, pr, d) in enumerate(zip(entries, prs, ds)):
        c, _, rs = collect(pr, d)
        ref = gc.reference(pr)
        if e['share'] is not None:
            c, want, bound = None, None, None                        # (checked with the entry that owns the destination)
        else:
            want, bound = ref['c'], ref['bound']
            for j in sharers[i]:                                     # the destination also received the products of these entries
                rj = gc.reference(prs[j])
                want, bound = want + rj['c'] - prs[j]['C0'].double(), bound + rj['bound_term']
        if kind == 'int':
            bound = None if bound is None else torch.zeros_like(bound)
        if c is not None:
            gc.check('rv_gemm_table_run ' + kind, e['name'], 'c', gc.err_ratio(c, want, bound), log=True)
        if e['rowsum']:
            brs = ref['bound_rs'] if kind == 'float' else torch.zeros_like(ref['bound_rs'])
            gc.check('rv_gemm_table_run ' + kind, e['name'], 'rs', gc.err_ratio(rs, ref['rs'], brs), log=True)


@pytest.mark.parametrize('name', list(gc.TABLES))
def test_table_entry_on_a_zeroed_destination_equals_the_direct_call(dev, name):
    """splitk = 1 and parked entries (an atomic split-K depends on the arrival order): one atomic add of the folded value onto 0"""
    entries, prs, ds = run_table(dev, name, 'float', zero=True)
    shared = {e['share'] for e in entries if e['share'] is not None}
    compared = 0
    for i, (e, pr, d) in enumerate(zip(entries, prs, ds)):
        if e['mode'] == 'atomic' or e['share'] is not None or i in shared:
            continue
        c, _, rs = collect(pr, d)
        direct, _, drs = run(dev, pr, zero=True, acc=0)
        assert torch.equal(c, direct), e['name']
        assert rs is None or torch.equal(rs, drs), e['name']
        compared += 1
    assert compared >= 1


# ---------------------------------------------------------------------------------------------------------------------
# refusals: -1, nothing launched, the destination untouched
# ---------------------------------------------------------------------------------------------------------------------
def _refused(dev, pr, d, args, what):
    lib = _lib()
    before = {k: _bits(d[k]).clone() for k in ('C', 'C2', 'rs') if d[k] is not None}
    rc = lib.invoke('rv_gemm', *args)
    torch.cuda.synchronize()
    assert rc == -1, (what, rc)
    assert lib.last_error(), what
    for k, b in before.items():
        assert torch.equal(_bits(d[k]), b), (what, k)


def _replace(args, **kw):
    names = ['A', 'sam', 'sak', 'B', 'sbk', 'sbn', 'C', 'scm', 'scn', 'C2', 'sc2m', 'sc2n', 'bias', 'M', 'N', 'K', 'act', 'accumulate', 'splitk',
             'batch', 'bsa', 'bsb', 'bsc', 'a_rowsum', 'ws', 'tickets', 'stream']
    a = list(args)
    for k, v in kw.items():
        a[names.index(k)] = v
    return tuple(a)


def test_gemm_refusals(dev):
    pr = gc.problem(gc.CASES['splitk K33 s2 parked all'], 'float')   # bias, C2, a_rowsum, a workspace: every pointer is live
    d = upload(dev, pr)
    ws = workspace(dev, pr, 2, True)
    ok = gemm_args(pr, d, ws)
    for what, kw in (('M = 0', {'M': 0}), ('N = 0', {'N': 0}), ('K = 0', {'K': 0}), ('splitk = 0', {'splitk': 0}), ('batch = 0', {'batch': 0}),
                     ('a_rowsum with batch > 1', {'batch': 2, 'C2': None}),
                     ('C2 with batch > 1', {'batch': 2, 'a_rowsum': None}),
                     ('atomic split-K with C2', {'ws': None}),
                     ('atomic split-K with act', {'ws': None, 'C2': None, 'act': 1}),
                     ('batch * splitk >= 65536', {'batch': 256, 'splitk': 256, 'C2': None, 'a_rowsum': None}),
                     ('batched atomic split-K without accumulate', {'batch': 2, 'ws': None, 'C2': None, 'a_rowsum': None, 'accumulate': 0})):
        _refused(dev, pr, d, _replace(ok, **kw), what)
    # ... and the same buffers still serve the accepted call
    _lib().call('rv_gemm', *ok)
    c, c2, rs = collect(pr, d)
    for key, ratio in gc.compare(pr, c, c2, rs).items():
        gc.check('rv_gemm after refusals', pr['case']['name'], key, ratio)


def test_gemm_table_refusals(dev):
    lib = _lib()
    pr = gc.problem(gc.CASES['splitk K33 s2 parked plain'], 'float')
    d = upload(dev, pr)
    a = gemm_args(pr, d, None)
    fill = (*a[:9], a[12], *a[13:16], 1, 1, *a[20:23], None, None)
    code = gc.table_layout([gc.case_regime(pr['case'], table=True)])['code']
    assert lib.invoke('rv_gemm_table_fill', None, *fill) == -1 and lib.last_error()
    nbytes = lib.load().rv_gemm_table_entry_bytes()
    host = torch.zeros(65 * nbytes, dtype=torch.uint8)
    for i in range(65):
        assert lib.invoke('rv_gemm_table_fill', host.data_ptr() + i * nbytes, *fill) == code
    fold = ctypes.c_long(-1)
    total = lib.invoke('rv_gemm_table_finalize', host.data_ptr(), 65, ctypes.addressof(fold))
    assert (total, fold.value) == (65 * 4, 0)
    table = host.to(dev)
    before = _bits(d['C']).clone()
    for what, args in (('65 entries', (table.data_ptr(), 65, total, 0, code, lib.stream())), ('no entries', (table.data_ptr(), 0, total, 0, code, lib.stream())),
                       ('no workgroups', (table.data_ptr(), 64, 0, 0, code, lib.stream())), ('a negative fold grid', (table.data_ptr(), 64, 256, -1, code, lib.stream()))):
        assert lib.invoke('rv_gemm_table_run', *args) == -1, what
    torch.cuda.synchronize()
    assert torch.equal(_bits(d['C']), before)
