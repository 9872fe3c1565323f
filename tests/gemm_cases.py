"""Case table, launch arithmetic, inputs and references for the generic-stride fp32 GEMM of csrc/gemm.hip.

What gemm_args_make, rv_gemm, gemm_tile, gemm_epilogue, gemm_fold_tile, rv_gemm_table_fill and rv_gemm_table_finalize decide on
the host or per workgroup (operand orientation with its tie rule, 16-byte or scalar loads and their scalar tails, the k slices of
a split-K, the store path, the zero-fill and fold launches, the workspace layout, the table prefixes, the big-tile choice) is
restated here in Python (`gemm_regime`, `table_layout`), and every case below carries the regime it is meant to reach.
tests/test_gemm_cases.py asserts on the CPU that each case lands in its regime, that the cases together reach every regime, that
torch's float32 CPU product meets the derived bound and that emulated kernel faults miss it; tests/test_gemm_regimes_gpu.py runs
the kernels through the C ABI.  A case edit can therefore not fall back to the easy path silently.

Detection is by construction.  Every case runs two problems:
  * the INTEGER problem: all of A, B, bias, the start values of C and a_rowsum drawn from {+-1, +-2, +-3}.  Every partial sum is an
    integer below 2^24 (K <= 300), so the float32 result is exact in ANY summation order, atomics included, and the device result
    must equal the int64 reference with `==`: one dropped, doubled or misplaced term moves a sum by a non-zero integer;
  * the FLOAT problem: magnitudes uniform in [0.5, 1], random sign, against float64 of the same float32 inputs under the forward
    bound of a K-term fused multiply-add chain plus the slice adds, the bias and the accumulate, in any order, per element:
        |got - ref| <= 1.01 (K + splitk + 3) 2^-24 (|A| @ |B| + |bias| + |C0|)[m, n]
    (with the sigmoid: a quarter of it -- the sigmoid's largest slope -- plus TOL for __expf).
Operands live in wider buffers whose padding -- the skipped elements of a stride-2 view included -- is NaN: an over-read that reaches
a sum shows, and stays inside the allocation.  C, C2 and a_rowsum live in wider buffers prefilled with a NaN bit pattern (the live
region: NaN, or the start value when accumulating) and the padding must come back bit-unchanged; split-K workspaces are NaN-filled.
"""
import json
import os

import torch

import parity_tol

TOL = 2e-5                      # __expf in the sigmoid epilogue (tests/test_ops_gpu.py)
U = 2.0 ** -24                  # unit roundoff of float32
PAD_BITS = 0x7FC5EED5           # padding of destinations: a NaN with a recognisable payload (int32 view)

GBM, GBN, GBK = 64, 64, 32      # csrc/gemm.hip
SLOT_FLOATS = 4 * 256 * 4       # one parked 64 x 64 tile: 4 fragments x 256 threads x f32x4
FOLD_WIDTH = 4                  # slices whose loads gemm_fold_tile keeps in flight together


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def kslices(K, splitk):
    """mirrors kper / k_begin / k_end of gemm_tile: (kper, [(k_begin, k_end)] per slice; k_begin >= k_end: an empty slice)"""
    kper = cdiv(cdiv(K, splitk), GBK) * GBK
    return kper, [(z * kper, min(K, z * kper + kper)) for z in range(splitk)]


def workspace_bytes(M, N, splitk, batch):
    """mirrors rv_gemm_splitk_workspace_bytes"""
    if splitk <= 1:
        return 0
    return batch * splitk * cdiv(M, GBM) * cdiv(N, GBN) * SLOT_FLOATS * 4 + splitk * M * 4


def big_choice(policy, M, N, eligible):
    """mirrors the block-tile policy of rv_gemm: None (64 x 64), '128x128' or '128x64'"""
    if not policy or not eligible:
        return None
    if policy == 2:
        return '128x128'
    if policy == 3:
        return '128x64'
    wg128, wg64 = cdiv(M, 128) * cdiv(N, 128), cdiv(M, 128) * cdiv(N, 64)
    if wg128 >= 512 and cdiv(N, 128) * 128 * 10 <= cdiv(N, 64) * 64 * 11:
        return '128x128'
    return '128x64' if wg64 >= 384 else None


def gemm_regime(M, N, K, sam, sak, sbk, sbn, scm, scn, c2=False, bias=False, act=0, accumulate=0, splitk=1, batch=1, parked=False,
                a_rowsum=False, table=False):
    """What one rv_gemm call (table = True: one rv_gemm_table_fill entry) with these arguments does.  parked: splitk_ws is given."""
    parked = bool(parked) and splitk > 1
    if table:
        c2, act, accumulate = False, 0, 1
    a_kfast, b_kfast = sak <= sam, sbk <= sbn                        # (a tie counts as k-fast)
    a_vec = (sak if a_kfast else sam) == 1                           # unit stride along the fast dimension is all it takes: no alignment demanded
    b_vec = (sbk if b_kfast else sbn) == 1
    kper, sl = kslices(K, splitk)
    live = [(k0, k1) for k0, k1 in sl if k0 < k1]
    ktiles = [cdiv(k1 - k0, GBK) if k0 < k1 else 0 for k0, k1 in sl]
    k_tail = any((k1 - k0) % 4 for k0, k1 in live)

    def tail(vec, kfast, rows):
        if not vec:
            return None
        if kfast:
            return 'k' if k_tail else None
        return 'row' if rows % 4 else None
    atomic = (splitk > 1 and not parked) or table
    vec_ok = scn == 1 and not c2 and not atomic
    tm, tn = cdiv(M, GBM), cdiv(N, GBN)
    mode = 'single' if splitk == 1 else ('parked' if parked else 'atomic')
    eligible = a_kfast and b_kfast and splitk == 1 and batch == 1 and not a_rowsum and not c2 and sak == 1 and sbk == 1 and scn == 1 \
        and M >= 128 and not table
    return {
        'orient': (a_kfast, b_kfast), 'a_vec': a_vec, 'b_vec': b_vec,
        'a_tail': tail(a_vec, a_kfast, M), 'b_tail': tail(b_vec, b_kfast, N),
        'tiles': (tm, tn), 'partial': (M % GBM != 0, N % GBN != 0),
        'kper': kper, 'slices': sl, 'live_slices': len(live), 'empty_slices': splitk - len(live),
        'ktiles': ktiles, 'prefetch': any(t > 1 for t in ktiles), 'one_tile_slice': any(t == 1 for t in ktiles),
        'mode': mode, 'fold_groups': cdiv(splitk, FOLD_WIDTH) if parked else 0,
        # the store of a quad of four n: 16 bytes where the whole quad is inside N, else (and for every quad of the other paths) scalar
        'store': 'atomic' if atomic else ('vec' if vec_ok and N >= 4 else 'scalar'), 'partial_quad': N % 4 != 0,
        'zero_fill': splitk > 1 and not parked and not accumulate and not table, 'fold': parked,
        'bias_once': bool(bias) and mode == 'atomic',                # only the slice kz = 0 adds the bias
        'grid': (tn, tm, splitk * batch), 'fold_grid': (tn, tm, batch) if parked else None,
        'rowsum_idle_columns': bool(a_rowsum) and tn > 1,            # workgroups with bx > 0 exist and must not add
        'ws_bytes': workspace_bytes(M, N, splitk, batch) if parked else 0,
        'rs_offset': batch * splitk * tm * tn * SLOT_FLOATS if parked else None,       # in floats, inside the workspace
        'big': {p: big_choice(p, M, N, eligible) for p in (0, 2, 3)},
    }


def table_layout(regimes):
    """mirrors rv_gemm_table_fill / rv_gemm_table_finalize: the workgroup prefixes of both grouped launches and the orientation code"""
    block0, fold0, total, ftotal = [], [], 0, 0
    for r in regimes:
        tn, tm, z = r['grid']
        block0.append(total)
        fold0.append(ftotal)
        total += tn * tm * z
        ftotal += r['fold_grid'][0] * r['fold_grid'][1] * r['fold_grid'][2] if r['fold'] else 0
    codes = {(1 if r['orient'][0] else 0) | (2 if r['orient'][1] else 0) for r in regimes}
    assert len(codes) == 1, 'all entries of one table have the same operand orientation'
    return {'block0': block0, 'fold0': fold0, 'blocks': total, 'fold_blocks': ftotal, 'code': codes.pop()}


# ---------------------------------------------------------------------------------------------------------------------
# memory layouts
# ---------------------------------------------------------------------------------------------------------------------
def operand_layout(rows, cols, fast, place):
    """(offset, row stride, column stride) in floats of a rows x cols matrix whose `fast` dimension ('row' | 'col') is the quick one.
    dense; 'offset': a view into a wider buffer at an odd float offset with an odd row stride; 'stride2': every other float."""
    nf = cols if fast == 'col' else rows
    off, fs, ld = {'dense': (0, 1, nf), 'offset': (3, 1, nf + 1 + nf % 2), 'stride2': (1, 2, 2 * nf + 1)}[place]
    return (off, ld, fs) if fast == 'col' else (off, fs, ld)


def dest_layout(M, N, dest):
    """(offset, scm, scn): dense, a column slice of a wider buffer (cat[:, :N]), or transposed"""
    return {'dense': (0, N, 1), 'slice': (0, N + 5, 1), 'trans': (2, 1, M + 1)}[dest]


def extent(rows, cols, s_row, s_col):
    return (rows - 1) * s_row + (cols - 1) * s_col + 1


# ---------------------------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------------------------
ORIENTS = {'kk': (True, True), 'km': (True, False), 'mk': (False, True), 'mm': (False, False)}     # (A k-fast, B k-fast)
PLACES = ('dense', 'offset', 'stride2')

# shape -> what it means for the tiling (literal, not computed): tiles (m, n), partial edge tiles, k-tiles at splitk 1, and
# whether a 16-byte load along k / m / n ends in a scalar tail
SHAPES = {
    (1, 1, 1): {'tiles': (1, 1), 'partial': (True, True), 'ktiles': [1], 'tails': (True, True, True), 'quad': True},
    (64, 64, 32): {'tiles': (1, 1), 'partial': (False, False), 'ktiles': [1], 'tails': (False, False, False), 'quad': False},
    (65, 67, 33): {'tiles': (2, 2), 'partial': (True, True), 'ktiles': [2], 'tails': (True, True, True), 'quad': True},
    (130, 229, 70): {'tiles': (3, 4), 'partial': (True, True), 'ktiles': [3], 'tails': (True, True, True), 'quad': True},
    (70, 88, 229): {'tiles': (2, 2), 'partial': (True, True), 'ktiles': [8], 'tails': (True, True, False), 'quad': False},
}

CASES = {}


def _case(name, shape, orient='kk', place='dense', dest='dense', c2=False, bias=False, act=0, acc=0, splitk=1, mode='single', batch=1,
          rowsum=False, shared_b=False, a_slices=False, regime=None):
    assert name not in CASES, name
    assert mode == ('single' if splitk == 1 else mode) and mode in ('single', 'atomic', 'parked')
    CASES[name] = {'name': name, 'seed': len(CASES) + 1, 'shape': shape, 'orient': orient, 'place': place, 'dest': dest, 'c2': c2, 'bias': bias,
                   'act': act, 'acc': acc, 'splitk': splitk, 'mode': mode, 'batch': batch, 'rowsum': rowsum, 'shared_b': shared_b,
                   'a_slices': a_slices, 'regime': regime or {}}


def _shape_regime(shape, orient, place):
    """the label of one (shape, orientation, placement) of the first group, put together from the literal tables above"""
    s, (ak, bk) = SHAPES[shape], ORIENTS[orient]
    if shape == (1, 1, 1) and place == 'dense':
        ak = bk = True                                               # all strides are 1: the tie rule `<=` makes both operands k-fast
    vec = place != 'stride2'
    tk, tmm, tnn = s['tails']
    r = {'orient': (ak, bk), 'a_vec': vec, 'b_vec': vec, 'tiles': s['tiles'], 'partial': s['partial'], 'ktiles': s['ktiles'],
         'a_tail': (('k' if tk else None) if ak else ('row' if tmm else None)) if vec else None,
         'b_tail': (('k' if tk else None) if bk else ('row' if tnn else None)) if vec else None,
         'store': 'vec' if shape[1] >= 4 else 'scalar', 'partial_quad': s['quad'], 'mode': 'single', 'zero_fill': False, 'fold': False,
         'prefetch': s['ktiles'][0] > 1, 'one_tile_slice': s['ktiles'][0] == 1, 'big': {0: None, 2: None, 3: None}}
    if shape[0] >= 128 and orient == 'kk' and place != 'stride2':
        r['big'] = {0: None, 2: '128x128', 3: '128x64'}
    return r


# 1. every shape in all four orientations and three operand placements
for _s in SHAPES:
    for _o in ORIENTS:
        for _p in PLACES:
            _case('shape %dx%dx%d %s %s' % (_s + (_o, _p)), _s, _o, _p, regime=_shape_regime(_s, _o, _p))

# 2. destinations x bias x act x accumulate (one past every edge; K = 33 keeps the sigmoid off its flat ends)
_STORE = {'dense': 'vec', 'slice': 'vec', 'trans': 'scalar', 'c2': 'scalar'}
for _d in ('dense', 'slice', 'trans', 'c2'):
    for _b in (False, True):
        for _a in (0, 1):
            for _acc in (0, 1):
                _case('dest %s bias%d act%d acc%d' % (_d, _b, _a, _acc), (65, 67, 33), 'kk', 'dense', 'dense' if _d == 'c2' else _d,
                      c2=_d == 'c2', bias=_b, act=_a, acc=_acc, regime={'store': _STORE[_d], 'partial_quad': True, 'mode': 'single'})
    _case('dest %s mm offset all' % _d, (70, 88, 229), 'mm', 'offset', 'dense' if _d == 'c2' else _d, c2=_d == 'c2', bias=True, act=1, acc=1,
          regime={'store': _STORE[_d], 'partial_quad': False, 'orient': (False, False), 'a_tail': 'row', 'b_tail': None})

# 3. split-K at K = 229 and K = 33: literal slices per splitk
_SLICES = {
    (229, 2): [(0, 128), (128, 229)], (229, 3): [(0, 96), (96, 192), (192, 229)],
    (229, 5): [(0, 64), (64, 128), (128, 192), (192, 229), (256, 229)],
    (229, 6): [(0, 64), (64, 128), (128, 192), (192, 229), (256, 229), (320, 229)],
    (229, 8): [(32 * z, min(229, 32 * z + 32)) for z in range(8)],
    (33, 2): [(0, 32), (32, 33)], (33, 3): [(0, 32), (32, 33), (64, 33)],
    (33, 5): [(0, 32), (32, 33)] + [(32 * z, 33) for z in range(2, 5)],
    (33, 6): [(0, 32), (32, 33)] + [(32 * z, 33) for z in range(2, 6)],
    (33, 8): [(0, 32), (32, 33)] + [(32 * z, 33) for z in range(2, 8)],
}
_EMPTY = {(229, 2): 0, (229, 3): 0, (229, 5): 1, (229, 6): 2, (229, 8): 0, (33, 2): 0, (33, 3): 1, (33, 5): 3, (33, 6): 4, (33, 8): 6}
for _i, ((_K, _sk), _sl) in enumerate(_SLICES.items()):
    _shape = (70, 88, 229) if _K == 229 else (65, 67, 33)
    _o = list(ORIENTS)[_i % 4]
    _pl = PLACES[_i % 2]                                             # dense / offset: 16-byte loads whose last k quad of a ragged slice is scalar
    _r = {'slices': _sl, 'empty_slices': _EMPTY[(_K, _sk)], 'orient': ORIENTS[_o]}
    _case('splitk K%d s%d atomic acc' % (_K, _sk), _shape, _o, _pl, 'slice', bias=True, acc=1, splitk=_sk, mode='atomic',
          regime=dict(_r, mode='atomic', store='atomic', zero_fill=False, fold=False, bias_once=True))
    _case('splitk K%d s%d atomic zero' % (_K, _sk), _shape, _o, _pl, 'trans', bias=True, acc=0, splitk=_sk, mode='atomic',
          regime=dict(_r, mode='atomic', store='atomic', zero_fill=True, fold=False, bias_once=True))
    _case('splitk K%d s%d parked all' % (_K, _sk), _shape, _o, _pl, 'dense', c2=True, bias=True, acc=1, splitk=_sk, mode='parked', rowsum=True,
          regime=dict(_r, mode='parked', store='scalar', zero_fill=False, fold=True, fold_groups=1 if _sk <= 4 else 2,
                      rowsum_idle_columns=True))
    _case('splitk K%d s%d parked all sigmoid' % (_K, _sk), _shape, _o, _pl, 'slice', c2=True, bias=True, act=1, acc=1, splitk=_sk, mode='parked',
          rowsum=True, regime=dict(_r, mode='parked', store='scalar', fold=True, fold_groups=1 if _sk <= 4 else 2))
    _case('splitk K%d s%d parked plain' % (_K, _sk), _shape, _o, _pl, 'slice', splitk=_sk, mode='parked',
          regime=dict(_r, mode='parked', store='vec', fold=True, fold_groups=1 if _sk <= 4 else 2))

# 4. a_rowsum: N above 64 (workgroups with bx > 0 must not add), M partial; A = dY^T is M-fast in the product
for _shape, _o in (((70, 88, 229), 'mk'), ((130, 229, 70), 'mm'), ((65, 67, 33), 'kk')):
    _t = '%dx%dx%d' % _shape
    _case('rowsum %s s1' % _t, _shape, _o, 'offset', 'dense', acc=1, rowsum=True,
          regime={'rowsum_idle_columns': True, 'mode': 'single', 'partial': (True, True), 'orient': ORIENTS[_o]})
    _case('rowsum %s atomic' % _t, _shape, _o, 'offset', 'dense', acc=1, splitk=2, mode='atomic', rowsum=True,
          regime={'rowsum_idle_columns': True, 'mode': 'atomic', 'store': 'atomic'})
    _case('rowsum %s parked' % _t, _shape, _o, 'offset', 'dense', acc=0, splitk=3, mode='parked', rowsum=True,
          regime={'rowsum_idle_columns': True, 'mode': 'parked', 'fold': True, 'fold_groups': 1})

# 5. batch > 1 outside a table
_case('batch3 s1', (65, 67, 33), 'kk', 'offset', 'slice', bias=True, batch=3, regime={'grid': (2, 2, 3), 'mode': 'single'})
_case('batch3 s1 mm sigmoid', (65, 67, 33), 'mm', 'dense', 'trans', bias=True, act=1, acc=1, batch=3, regime={'grid': (2, 2, 3), 'store': 'scalar'})
_case('batch3 atomic acc', (65, 67, 70), 'mk', 'dense', 'dense', acc=1, splitk=2, mode='atomic', batch=3,
      regime={'grid': (2, 2, 6), 'mode': 'atomic', 'zero_fill': False, 'slices': [(0, 64), (64, 70)]})
_case('batch3 parked', (65, 67, 70), 'km', 'offset', 'dense', bias=True, acc=1, splitk=3, mode='parked', batch=3,
      regime={'grid': (2, 2, 9), 'fold_grid': (2, 2, 3), 'mode': 'parked', 'empty_slices': 0, 'ws_bytes': 3 * 3 * 4 * 16384 + 3 * 65 * 4})
_case('batch3 shared B', (65, 67, 33), 'km', 'dense', 'dense', acc=1, batch=3, shared_b=True, regime={'grid': (2, 2, 3)})
_case('batch3 A column slices', (31, 31, 70), 'mk', 'dense', 'dense', acc=1, batch=3, a_slices=True,      # the attention's (dh, 31, dh*31)
      regime={'grid': (1, 1, 3), 'orient': (False, True), 'a_tail': 'row'})
_case('batch3 A k slices parked', (31, 31, 70), 'kk', 'dense', 'dense', splitk=2, mode='parked', batch=3, a_slices=True,
      regime={'grid': (1, 1, 6), 'fold_grid': (1, 1, 3)})

# 6. the opt-in big tiles: M of 128 and of 130, N partial against 128 and against 64, a K tail
for _M in (128, 130):
    for _N in (67, 229):
        for _n, _kw in (('bias', {'bias': True}), ('sigmoid', {'bias': True, 'act': 1}), ('acc', {'acc': 1})):
            _case('big %dx%dx70 %s' % (_M, _N, _n), (_M, _N, 70), 'kk', 'dense', 'slice' if _N == 67 else 'dense',
                  regime={'big': {0: None, 2: '128x128', 3: '128x64'}, 'ktiles': [3], 'a_tail': 'k', 'partial_quad': True}, **_kw)
BIG_CASES = [n for n in CASES if n.startswith('big ')]

# 7. tables: entries in launch order; every entry accumulates atomically into its destination (rv_gemm_table_fill).  `share`: the
# destination of an earlier entry of the table (same M, N).  Each of the four orientation tables is parked, unparked, parked, so the
# fold scan has to step over an entry that owns no fold workgroups.
def _entry(shape, splitk=1, parked=False, bias=False, batch=1, rowsum=False, place='dense', dest='dense', share=None):
    return {'shape': shape, 'splitk': splitk, 'mode': 'single' if splitk == 1 else ('parked' if parked else 'atomic'), 'bias': bias,
            'batch': batch, 'rowsum': rowsum, 'place': place, 'dest': dest, 'share': share, 'c2': False, 'act': 0, 'acc': 1,
            'shared_b': False, 'a_slices': False}


TABLES = {
    'kk parked unparked parked+rowsum': ('kk', [_entry((70, 88, 229), 3, True, bias=True), _entry((65, 67, 33), place='offset', dest='slice'),
                                                _entry((70, 88, 229), 5, True, rowsum=True, place='offset')],
                                         {'code': 3, 'block0': [0, 12, 16], 'fold0': [0, 4, 4], 'blocks': 36, 'fold_blocks': 8}),
    'km parked atomic-split parked-batch': ('km', [_entry((65, 67, 33), 2, True), _entry((70, 88, 229), 2, False, bias=True, dest='trans'),
                                                   _entry((31, 31, 70), 2, True, batch=3)],
                                            {'code': 1, 'block0': [0, 8, 16], 'fold0': [0, 4, 4], 'blocks': 22, 'fold_blocks': 7}),
    'mk parked unparked parked shared': ('mk', [_entry((70, 88, 229), 8, True, dest='slice'), _entry((130, 229, 70), place='stride2'),
                                                _entry((70, 88, 70), 2, True, dest='slice', share=0)],
                                         {'code': 2, 'block0': [0, 32, 44], 'fold0': [0, 4, 4], 'blocks': 52, 'fold_blocks': 8}),
    'mm parked unparked parked': ('mm', [_entry((65, 67, 33), 3, True, rowsum=True), _entry((1, 1, 1), place='offset'),
                                         _entry((70, 88, 229), 6, True, bias=True, place='offset', dest='trans')],
                                  {'code': 0, 'block0': [0, 12, 13], 'fold0': [0, 4, 4], 'blocks': 37, 'fold_blocks': 8}),
    'mk unparked first': ('mk', [_entry((65, 67, 33), rowsum=True), _entry((70, 88, 229), 3, True), _entry((65, 67, 33), share=0),
                                 _entry((64, 64, 32), 2, False)],
                          {'code': 2, 'block0': [0, 4, 16, 20], 'fold0': [0, 0, 4, 4], 'blocks': 22, 'fold_blocks': 4}),
}


def table_entries(name):
    """the entries of a table as case dicts (problem() and case_regime() take them)"""
    orient, entries, _ = TABLES[name]
    return [dict(e, name='%s #%d' % (name, i), orient=orient, seed=1000 + 16 * sorted(TABLES).index(name) + i, regime={}) for i, e in enumerate(entries)]


def case_args(case):
    """the strides of a case: {'A': (offset, sam, sak, bsa), 'B': (offset, sbk, sbn, bsb), 'C': (offset, scm, scn, bsc), 'C2': ...}"""
    (M, N, K), (ak, bk), batch = case['shape'], ORIENTS[case['orient']], case['batch']
    wide = batch if case['a_slices'] else 1                          # problem z of A: a slice along the fast dimension of one wide matrix
    if ak:
        off, sam, sak = operand_layout(M, K * wide, 'col', case['place'])
        ext = extent(M, K * wide, sam, sak)
    else:
        off, sam, sak = operand_layout(M * wide, K, 'row', case['place'])
        ext = extent(M * wide, K, sam, sak)
    bsa = (K * sak if ak else M * sam) if case['a_slices'] else (ext + 5 if batch > 1 else 0)
    out = {'A': (off, sam, sak, bsa), 'A_floats': off + (ext if case['a_slices'] else (batch - 1) * bsa + ext) + 4}
    off, sbk, sbn = operand_layout(K, N, 'row' if bk else 'col', case['place'])
    ext = extent(K, N, sbk, sbn)
    bsb = ext + 7 if batch > 1 and not case['shared_b'] else 0
    out.update(B=(off, sbk, sbn, bsb), B_floats=off + (batch - 1) * bsb + ext + 4)
    off, scm, scn = dest_layout(M, N, case['dest'])
    ext = extent(M, N, scm, scn)
    bsc = ext + 3 if batch > 1 else 0
    out.update(C=(off, scm, scn, bsc), C_floats=off + (batch - 1) * bsc + ext + 4)
    if case['c2']:                                                   # its own, transposed strides
        off2, s2m, s2n = (1, 1, M + 2) if scm != 1 else (1, N + 1, 1)
        out.update(C2=(off2, s2m, s2n, 0), C2_floats=off2 + extent(M, N, s2m, s2n) + 4)
    return out


def case_regime(case, table=False):
    (M, N, K), ar = case['shape'], case_args(case)
    _, sam, sak, _ = ar['A']
    _, sbk, sbn, _ = ar['B']
    _, scm, scn, _ = ar['C']
    return gemm_regime(M, N, K, sam, sak, sbk, sbn, scm, scn, c2=case['c2'], bias=case['bias'], act=case['act'], accumulate=case['acc'],
                       splitk=case['splitk'], batch=case['batch'], parked=case['mode'] == 'parked', a_rowsum=case['rowsum'], table=table)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references (CPU, seeded per case, cached, never modified by the tests)
# ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))
    return g


def _draw(g, kind, *shape):
    """int: {+-1, +-2, +-3}, never 0; float: magnitude uniform in [0.5, 1], random sign"""
    sign = (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    if kind == 'int':
        return sign * torch.randint(1, 4, shape, generator=g).float()
    return sign * (0.5 + 0.5 * torch.rand(shape, generator=g))


def _view(buf, off, shape, strides):
    return torch.as_strided(buf, shape, strides, off)


def _pad_buffer(n):
    buf = torch.empty(n, dtype=torch.float32)
    buf.view(torch.int32).fill_(PAD_BITS)
    return buf


_problems = {}


def problem(case, kind):
    """One problem of a case: the logical float32 tensors A [batch, M, K], B [batch or 1, K, N], bias [N], C0 [batch, M, N], rs0 [M] and
    the flat host buffers they live in (operands: NaN padding; destinations: PAD_BITS padding, the live region NaN or the start value)."""
    key = (case['name'], kind)
    if key in _problems:
        return _problems[key]
    (M, N, K), batch, ar = case['shape'], case['batch'], case_args(case)
    g = _gen(case['seed'], kind == 'int')
    nb = 1 if case['shared_b'] else batch
    pr = {'case': case, 'kind': kind, 'args': ar, 'A': _draw(g, kind, batch, M, K), 'B': _draw(g, kind, nb, K, N),
          'bias': _draw(g, kind, N) if case['bias'] else None, 'C0': _draw(g, kind, batch, M, N) if case['acc'] else None,
          'rs0': _draw(g, kind, M) if case['rowsum'] else None}
    off, sam, sak, bsa = ar['A']
    pr['A_buf'] = torch.full((ar['A_floats'],), float('nan'))
    _view(pr['A_buf'], off, (batch, M, K), (bsa, sam, sak)).copy_(pr['A'])
    off, sbk, sbn, bsb = ar['B']
    pr['B_buf'] = torch.full((ar['B_floats'],), float('nan'))
    _view(pr['B_buf'], off, (nb, K, N), (bsb, sbk, sbn)).copy_(pr['B'])
    if case['bias']:
        pr['bias_buf'] = torch.full((N + 4,), float('nan'))
        pr['bias_buf'][:N] = pr['bias']
    off, scm, scn, bsc = ar['C']
    pr['C_buf'] = _pad_buffer(ar['C_floats'])
    _view(pr['C_buf'], off, (batch, M, N), (bsc, scm, scn)).copy_(pr['C0'] if case['acc'] else torch.full((batch, M, N), float('nan')))
    if case['c2']:
        off, s2m, s2n, _ = ar['C2']
        pr['C2_buf'] = _pad_buffer(ar['C2_floats'])
        _view(pr['C2_buf'], off, (1, M, N), (0, s2m, s2n)).fill_(float('nan'))
    if case['rowsum']:
        pr['rs_buf'] = _pad_buffer(M + 6)
        pr['rs_buf'][1:1 + M] = pr['rs0']                            # (a_rowsum always accumulates)
    _problems[key] = pr
    return pr


def live(pr, which, buf):
    """the logical region of destination `which` ('C' | 'C2') inside `buf`, as a [batch, M, N] view"""
    (M, N, _), batch = pr['case']['shape'], pr['case']['batch']
    off, sm, sn, bs = pr['args'][which]
    return _view(buf, off, (batch if which == 'C' else 1, M, N), (bs, sm, sn))


def padding_intact(pr, which, buf):
    """every float of `buf` outside the logical region still holds PAD_BITS"""
    b = buf.detach().cpu().clone()
    if which == 'rs':
        b[1:1 + pr['case']['shape'][0]].view(torch.int32).fill_(PAD_BITS)
    else:
        live(pr, which, b.view(torch.int32)).fill_(PAD_BITS)
    return bool((b.view(torch.int32) == PAD_BITS).all().item())


def reference(pr, k_drop=0):
    """float64 (the integer problem: int64, exactly) of the float32 inputs, with the per-element bounds of the module docstring.
    -> {'pre', 'c', 'c2', 'rs', 'bound', 'bound_pre', 'bound_term', 'bound_c2', 'bound_rs'}.  c2 receives what C receives.  k_drop: leave the last terms out."""
    case = pr['case']
    K, sk = case['shape'][2] - k_drop, case['splitk']
    A, B = pr['A'][:, :, :K], pr['B'][:, :K, :]
    if pr['kind'] == 'int':
        pre = (A.long() @ B.long()).double()
    else:
        pre = A.double() @ B.double()
    mag = A.double().abs() @ B.double().abs()
    if case['bias']:
        pre = pre + pr['bias'].double()
        mag = mag + pr['bias'].double().abs()
    val = torch.sigmoid(pre) if case['act'] else pre
    c = val + pr['C0'].double() if case['acc'] else val
    scale = 1.01 * (case['shape'][2] + sk + 3) * U
    bound_term = scale * mag                                         # (without the start value: what a second entry adds to a shared C)
    if case['acc']:
        mag = mag + pr['C0'].double().abs()
    bound = bound_pre = scale * mag
    if case['act']:
        bound = bound / 4 + TOL
    out = {'pre': pre, 'bound_pre': bound_pre, 'bound_term': bound_term, 'c': c, 'bound': bound, 'c2': c, 'bound_c2': bound}
    if case['rowsum']:
        out['rs'] = A[0].double().sum(1) + pr['rs0'].double()
        out['bound_rs'] = scale * (A[0].double().abs().sum(1) + pr['rs0'].double().abs())
    return out


def err_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound in float64: 0 where they are equal (so a bound of 0 -- the integer problem is exact --
    asks for `==`), inf for a NaN or a difference against a zero bound"""
    got, ref = got.detach().double().cpu(), ref.double()
    d = (got - ref).abs()
    if bool(torch.isnan(d).any()):
        return float('inf')
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return r.max().item() if r.numel() else 0.0


def bounds(pr, ref):
    """the bounds the comparison applies: the integer problem without the sigmoid is exact"""
    if pr['kind'] == 'int' and not pr['case']['act']:
        z = torch.zeros_like(ref['bound'])
        return z, z, torch.zeros_like(ref['bound_rs']) if 'rs' in ref else None
    return ref['bound'], ref['bound_c2'], ref.get('bound_rs')


def compare(pr, c, c2=None, rs=None):
    """{'c': ratio, 'c2': ratio, 'rs': ratio} of results against reference(pr); <= 1 passes"""
    ref = reference(pr)
    b, b2, brs = bounds(pr, ref)
    out = {'c': err_ratio(c, ref['c'], b)}
    if pr['case']['c2']:
        out['c2'] = err_ratio(c2, ref['c2'], b2)
    if pr['case']['rowsum']:
        out['rs'] = err_ratio(rs, ref['rs'], brs if pr['kind'] == 'float' else torch.zeros_like(ref['bound_rs']))
    return out


def emulate(pr, fault=None, order='slices'):
    """float32 on the CPU.  order 'slices': the mirror's k slices, each `a @ b`, summed in k order; 'plain': one `a @ b`.
    fault: None | 'drop_k' (the last k column) | 'drop_row' (the last row of C is never stored) | 'skip_slice' (the last non-empty
    slice) | 'rowsum_per_ntile' (every column of workgroups adds the row sum).  -> (c, c2, rs) float32"""
    case = pr['case']
    (M, N, K), sk = case['shape'], case['splitk']
    A, B = pr['A'], pr['B']
    K_eff = K - 1 if fault == 'drop_k' else K
    if order == 'plain':
        acc = A[:, :, :K_eff] @ B[:, :K_eff, :]
    else:
        _, sl = kslices(K, sk)
        livesl = [(k0, min(k1, K_eff)) for k0, k1 in sl if k0 < min(k1, K_eff)]
        if fault == 'skip_slice':
            livesl = livesl[:-1]
        acc = torch.zeros(case['batch'], M, N)
        for k0, k1 in livesl:
            acc = acc + A[:, :, k0:k1] @ B[:, k0:k1, :]
    if case['bias']:
        acc = acc + pr['bias']
    if case['act']:
        acc = torch.sigmoid(acc)
    c = acc + pr['C0'] if case['acc'] else acc
    c = c.clone()
    if fault == 'drop_row':
        c[:, M - 1] = pr['C0'][:, M - 1] if case['acc'] else float('nan')
    rs = None
    if case['rowsum']:
        rows = A[0].sum(1)
        rs = pr['rs0'] + rows * (cdiv(N, GBN) if fault == 'rowsum_per_ntile' else 1)
    return c, c, rs


# ---------------------------------------------------------------------------------------------------------------------
# measuring and asserting
# ---------------------------------------------------------------------------------------------------------------------
# next to the loss-term errors of tests/parity_tol.py: the project's one directory for measured figures
_OUT = os.path.join(os.path.dirname(parity_tol._OUT), 'gemm_errors.jsonl')


def check(where, case, key, ratio, log=None):
    """Assert one measured ratio error / bound (<= 1) and (log = True: on the device) append it to gemm_errors.jsonl (see _OUT)."""
    ratio = float(ratio)
    if log:
        try:
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            with open(_OUT, 'a') as fh:
                fh.write(json.dumps({'where': where, 'case': case, 'key': key, 'ratio': ratio}) + '\n')
        except OSError:
            pass
    assert ratio <= 1.0, (where, case, key, ratio)                   # (inf -- a NaN, or an integer mismatch -- fails)
    return ratio
