"""Case table and launch arithmetic of the persistent 3x3 band kernel conv3x3_lds_k of csrc/conv.hip: what rv_conv_fwd runs for every 3x3
conv and 3x3 input gradient with Cin % 8 == 0 under algo 0 / 2, and forced as 0x2NM (4 waves), 0x3NM (8), 0x4NM (16), 0x7NM (12), with
TH << 12 rows per band and bit 20 for bf16 operands.

`band_regime` restates what conv_fwd_impl (the mode-0 branch), launch_conv3x3_lds (the tile search), conv3x3_lds_bytes, launch_conv3x3_lds_r
(the RV_L3 instance lists), band_grid (conv_band.h) and the prologue of the kernel decide; tests/conv_cases.py::conv_regime returns it for
the calls it used to label 'lds3x3'.  Inputs, references, comparisons and the error log are those of conv_cases.py: the INTEGER problem
(`==` against int64; exact under bf16 too, +-1 .. 3 are bf16 numbers) and the FLOAT problem under
    |got - ref| <= 1.01 (K + 3) 2^-24 (conv(|x|, |w|) + |bias| + |out0|),   K = 9 Cin,
for bf16 cases against float64 of the bf16-rounded (nearest even) x and w with 2K for K: the products of bf16 numbers are exact in float32,
the rounding of the matrix pipe's internal adds is not documented, so each of them is allowed a full ulp.

Not reachable from the host, so not mirrored and without a case: the kernel's nbuf == 3 (wait_vmcnt_le(ahead), the second
stage() of the prologue), skew (`late`) and xcd == 0 branches -- launch_conv3x3_lds_r sets nbuf = 2, skew = 0 and band_grid sets xcd = 1 --
and the RV_L3 instances (2, 8), (3, 4), (4, 4) at 16 waves, which the accumulator budget of the search (NT * MTW <= 8) never selects.
tests/test_band_cases.py checks all of this on the CPU, tests/test_band_regimes_gpu.py runs the kernel through the C ABI."""
import torch

import conv_cases as cc
from conv_cases import cdiv
from stream_cases import RV_BN_NREP

LDS_CAP = 150 * 1024            # launch_conv3x3_lds
LDS_TWO_PER_CU = 76 * 1024
FAM_NW = {2: 4, 3: 8, 4: 16, 7: 12}
NW_FAM = {nw: fam for fam, nw in FAM_NW.items()}
BF16_BIT = 1 << 20
MTS = {4: (8, 4, 2, 1), 8: (8, 4, 2, 1), 16: (8, 4, 2, 1), 12: (6, 5, 4, 3, 2, 1)}        # the search order of launch_conv3x3_lds
_POW2 = [(1, 1), (1, 2), (1, 4), (1, 8), (2, 1), (2, 2), (2, 4), (2, 8), (3, 1), (3, 2), (3, 4), (4, 1), (4, 2), (4, 4)]
RV_L3 = {4: _POW2, 8: _POW2, 16: _POW2,
         12: [(1, 3), (2, 3), (3, 3), (4, 3), (1, 5), (2, 5), (1, 6), (2, 6), (1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (4, 2), (1, 4), (2, 4)]}
TXF = 4                         # x staging slots planned in registers


def budget_ok(nw, nt, mt):
    """the accumulator budget of the search"""
    return not (nt * mt > 16 or (nw >= 12 and nt * mt > (8 if nw == 16 else 12)) or (nw == 12 and ((mt > 3 and nt > 2) or (nt == 3 and mt != 3))))


REACHABLE = {nw: [t for t in RV_L3[nw] if budget_ok(nw, *t)] for nw in RV_L3}


def lds_bytes(R, NT, TH, W, nchunk):
    """mirrors conv3x3_lds_bytes: two input units, one or two weight units"""
    return (2 * (TH + 2) * (W + 2) * 4 * R + (2 if nchunk > 1 else 1) * 9 * NT * 64 * R) * 4


def xcd_remap(bid, n):
    """mirrors xcd_remap (common.h)"""
    q, r, x, k = n >> 3, n & 7, bid & 7, bid >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + k


def search(R, nw, ntile_n, nchunk, B, H, W, force_nt=0, force_mt=0, force_th=0):
    """mirrors the loop of launch_conv3x3_lds -> (best or None, the reason each candidate that passed the forced filter was dropped for)"""
    best, best_score, dropped = None, -1, []
    for nt in (4, 3, 2, 1):
        if force_nt and nt != force_nt:
            continue
        if ntile_n % nt:
            dropped.append('ntile_n % NT')
            continue
        for mt in MTS[nw]:
            if force_mt and mt != force_mt:
                continue
            if not budget_ok(nw, nt, mt):
                dropped.append('accumulator budget')
                continue
            slots_th = (mt * 16 * nw) // W
            th, th_from = (H, 'H') if slots_th > H else (slots_th, 'slots')
            if force_th:
                if force_th > th:
                    dropped.append('force_th')
                    continue
                th, th_from = force_th, 'force_th'
            if th < 1:
                dropped.append('row wider than the tile slots')
                continue
            lds = lds_bytes(R, nt, th, W, nchunk)
            if lds > LDS_CAP:
                dropped.append('lds')
                continue
            wpc = 2 if (lds <= LDS_TWO_PER_CU and nw == 4) else 1
            bands = B * cdiv(H, th) * (ntile_n // nt)
            slots = 256 * wpc
            rounds = cdiv(bands, slots)
            fill = (bands * 100) // (rounds * slots)
            reuse = (nt * mt * 100) // (nt + mt)
            score = fill * (50 + reuse)
            if score > best_score:
                best_score, best = score, {'NT': nt, 'MTW': mt, 'TH': th, 'th_from': th_from, 'wpc': wpc, 'lds': lds, 'score': score}
    return best, dropped


def band_regime(B, H, W, Cin, Cout, in_ld=None, out_ld=None, algo=0, bias=True, accumulate=0, stats=None, z_ld=None, in_off=0, out_off=0):
    """What one mode-0 rv_conv_fwd call with Cin % 8 == 0, Cout > 2 and an algo outside the direct (0x1NM, 0x5NM, 1) families does.
    -> {'refused': reason} or the regime (of conv_mfma_k, from conv_cases.conv_regime, where nothing fits and the default falls through)."""
    in_ld = Cin if in_ld is None else in_ld
    out_ld = Cout if out_ld is None else out_ld
    z_ld = Cout if z_ld is None else z_ld
    R = cc.frag_R(Cin)
    assert R and Cout > 2
    if stats == 'z_only':
        return {'refused': 'bn_z without bn_sums'}
    if not (in_ld % R == 0 and (4 * in_off) % (4 * R) == 0):
        return {'refused': 'in alignment'}
    bf = bool(algo & BF16_BIT) and R == 4                            # bit 20 at R = 2: ignored
    algo &= ~BF16_BIT
    fam, f_nt, f_mt, f_th = (algo >> 8) & 15, (algo >> 4) & 15, algo & 15, (algo >> 12) & 255
    assert fam in (0, 2, 3, 4, 7) and algo != 1, 'only the band kernel is mirrored (the Winograd families are not)'
    forced = fam in FAM_NW
    nw = FAM_NW[fam] if forced else 4
    ntile_n, nchunk = cdiv(Cout, 16), Cin // (4 * R)
    if forced:
        best, dropped = search(R, nw, ntile_n, nchunk, B, H, W, f_nt, f_mt, f_th)
    else:
        best, dropped = search(R, 4, ntile_n, nchunk, B, H, W)
    if best is not None and (best['NT'], best['MTW']) not in RV_L3[nw]:
        best, dropped = None, ['no instance']                        # launch_conv3x3_lds_r returns RV_EUNSUPPORTED
    if best is None:
        if forced:
            return {'refused': 'forced tile: ' + (dropped[0] if len(set(dropped)) == 1 else 'nothing fits')}
        # the default falls through to conv_mfma_k with choose_tiles, as algo 1 does
        reg = cc.conv_regime(0, B, H, W, Cin, H, W, Cout, in_ld=in_ld, out_ld=out_ld, algo=1, bias=bias, accumulate=accumulate, stats=stats, z_ld=z_ld,
                             in_off=in_off, out_off=out_off)
        return dict(reg, fell_through=True)
    NT, MTW, TH = best['NT'], best['MTW'], best['TH']
    # band_grid
    nbands = cdiv(H, TH)
    total = B * nbands
    nsplit = ntile_n // NT
    wgs = min(max((256 * best['wpc']) // nsplit, 1), total)
    bpw = cdiv(total, wgs)
    wgs = cdiv(total, bpw)
    grid = wgs * nsplit
    runs = [(g * bpw, min((g + 1) * bpw, total)) for g in range(wgs)]
    # the kernel's prologue
    PPI = 64 // R
    ipr = cdiv(W, PPI)
    nx = (TH + 2) * ipr
    FPI = 4 // R
    NWF = cdiv(9 * NT, FPI)
    last_rows = H - (nbands - 1) * TH
    ntile_full, ntile_last = cdiv(TH * W, 16), cdiv(last_rows * W, 16)
    vec_out = out_ld % 4 == 0 and (4 * out_off) % 16 == 0
    stores, z_load = set(), set()
    for co0 in range(0, ntile_n * 16, 4):                            # one quad of four output channels per lane group and n-tile
        if co0 >= Cout:
            stores.add('skip')
            continue
        stores.add('scalar' if not vec_out else ('vec' if co0 + 3 < Cout else 'tail'))
        if stats == 'z':
            z_load.add('scalar_ld' if z_ld % 4 else ('vec' if co0 + 3 < Cout else 'scalar_tail'))
    return {
        'refused': None, 'kernel': 'band', 'fell_through': False, 'R': R, 'NW': nw, 'tile': (NT, MTW), 'forced': forced, 'bf': bf, 'form': (R, nw, NT, MTW, bf),
        'TH': TH, 'th_from': best['th_from'], 'lds_bytes': best['lds'], 'wgs_per_cu': best['wpc'], 'score': best['score'],
        'nchunk': nchunk, 'ntile_n': ntile_n, 'nbands': nbands, 'total_bands': total, 'nsplit': nsplit, 'bands_per_wg': bpw, 'grid': grid, 'runs': runs,
        'xcd': grid >= 9, 'short_last_run': total % bpw != 0, 'run_crosses_image': any(lo // nbands != (hi - 1) // nbands for lo, hi in runs),
        'PPI': PPI, 'ipr': ipr, 'row_tail': W % PPI != 0, 'nx': nx, 'idle_stagers': nx < nw, 'planned_only': nx <= TXF * nw, 'overflow_loop': nx > TXF * nw,
        'NWF': NWF, 'TW': cdiv(NWF, nw), 'w_half_instr': R == 2 and (9 * NT) % 2 == 1, 'weights': 'once' if nchunk == 1 else 'per_unit',
        'last_band_rows': last_rows, 'short_last_band': last_rows < TH, 'one_band_image': nbands == 1, 'H1': H == 1,
        'ntile': (ntile_full, ntile_last), 'partial_tile': (TH * W) % 16 != 0 or (last_rows * W) % 16 != 0, 'tile_spans_rows': W % 16 != 0,
        'idle_tile_slots': nw * MTW - ntile_full, 'idle_waves': max(0, nw - ntile_full),
        'vec_out': vec_out, 'stores': stores, 'z_load': z_load or None, 'stats': {None: None, 'sums': 'fwd', 'z': 'bn_z'}[stats],
        'replicas': {i % RV_BN_NREP for i in range(grid)} if stats else None, 'K': 9 * Cin, 'f': 0}


def forced(nw, nt, mt, th=0, bf=0):
    return NW_FAM[nw] << 8 | nt << 4 | mt | th << 12 | (BF16_BIT if bf else 0)


def base_algo(case):
    """the four-wave (1, 1) tile with one row per band the bit identities compare with: each output element is one chain ordered by chunk, tap, k
    wherever its lane sits.  (0x211 holds rows of up to 64 pixels.)"""
    assert case['W'] <= 64
    return 0x211 | (case['algo'] & BF16_BIT)


# ---------------------------------------------------------------------------------------------------------------------
# case table (the dictionaries are those of conv_cases.CASES, with seeds from 1000 on: the pack layout alternates and every third pack is flipped, as there)
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}


def _case(name, grid, cin, cout, algo=0, bias=True, acc=0, in_pad=0, out_pad=0, stats=None, z_pad=0, refusal=None, regime=None, in_off=0, out_off=0, bias_off=0, z_off=0, coef_off=0):
    assert name not in CASES, name
    B, H, W = grid
    CASES[name] = {'name': 'band ' + name, 'seed': 1000 + len(CASES), 'mode': 0, 'B': B, 'H': H, 'W': W, 'Ho': H, 'Wo': W, 'cin': cin, 'cout': cout, 'algo': algo,
                   'bias': bias, 'acc': acc, 'in_pad': in_pad, 'out_pad': out_pad, 'bias_off': bias_off, 'stats': stats, 'z_pad': z_pad, 'slope': 0.01,
                   'in_off': in_off, 'z_off': z_off, 'coef_off': coef_off, 'out_off': out_off, 'refusal': refusal, 'regime': regime or {}}


# 1. every reachable RV_L3 instance of every NW at R = 4, over pixel grids of one pixel, 70 pixels in one band per image (tiles span rows), rows of
# 15, 16, 17 and 33 pixels, and 7 rows in forced bands of 3 (a last band of one row); plain / accumulate / no bias, dense / +4 / +1 destinations,
# no / forward / backward statistics and 1, 2, 4 n-splits rotate
GRIDS = [((2, 5, 7), 0), ((1, 1, 1), 0), ((2, 3, 15), 0), ((2, 4, 16), 0), ((2, 3, 17), 0), ((2, 3, 33), 0), ((2, 7, 9), 3)]
_VAR = [{}, {'acc': 1}, {'bias': False}]


def _rotated(i, nw, nt, mt, cins, R):
    grid, th = GRIDS[i % len(GRIDS)]
    nsplit = (1, 1, 2, 1, 4)[i % 5]
    if nt >= 3 and nsplit == 4:
        nsplit = 2
    kw = dict(_VAR[i % 3], out_pad=(0, 4, 1)[(i // 3) % 3], stats=(None, 'sums', 'z')[(i // 2) % 3])
    if kw['stats'] == 'z' and i % 4 == 0:
        kw['z_pad'] = 4
    cin = cins[i % len(cins)]
    lab = {'kernel': 'band', 'R': R, 'NW': nw, 'tile': (nt, mt), 'forced': True, 'bf': False, 'nsplit': nsplit, 'nchunk': cin // (4 * R),
           'th_from': 'force_th' if th else ('H' if mt * 16 * nw // grid[2] > grid[1] else 'slots')}
    _case('R%d nw%d nt%d mt%d %dx%dx%d %d->%d' % ((R, nw, nt, mt) + grid + (cin, 16 * nt * nsplit)), grid, cin, 16 * nt * nsplit, forced(nw, nt, mt, th), regime=lab, **kw)


_i = 0
for _nw in (4, 8, 12, 16):
    for _nt, _mt in REACHABLE[_nw]:
        _rotated(_i, _nw, _nt, _mt, (16, 32, 48), 4)
        _i += 1
# ... and at R = 2 the instances reconvat_amd/tuned_plans.json ships (0x312, 0x314, 0x713 .. 0x716, 0x733) and two or three more per NW
R2_SHIPPED = [(8, 1, 2), (8, 1, 4), (12, 1, 3), (12, 1, 4), (12, 1, 5), (12, 1, 6), (12, 3, 3)]
for _nw, _nt, _mt in R2_SHIPPED + [(4, 1, 1), (4, 2, 2), (4, 3, 4), (8, 4, 4), (8, 2, 8), (12, 2, 6), (12, 4, 3), (16, 1, 1), (16, 2, 4), (16, 3, 2)]:
    _rotated(_i, _nw, _nt, _mt, (8, 24), 2)
    _i += 1

# 2. persistent runs: a forced TH = 1 on 2 x 65 rows, Cout = 64 at NT = 1 (four n-splits share the 256 slots: 64 workgroups for 130 bands) -- runs of
# three bands, one of them over the image boundary, a last run of one band, 176 workgroups; with one chunk (weights staged once) and with three
# (the staging and the compute cursor wrap chunks while they cross the image); plain, accumulating into a padded destination, and with both statistics
_RUN = {'kernel': 'band', 'NW': 8, 'tile': (1, 1), 'TH': 1, 'th_from': 'force_th', 'nbands': 65, 'total_bands': 130, 'nsplit': 4, 'bands_per_wg': 3, 'grid': 176,
        'xcd': True, 'short_last_run': True, 'run_crosses_image': True, 'idle_stagers': True, 'ntile': (1, 1), 'idle_waves': 7}
_case('run 16->64', (2, 65, 7), 16, 64, 0x1311, regime=dict(_RUN, weights='once', R=4))
_case('run 48->64 acc out_ld+4', (2, 65, 7), 48, 64, 0x1311, acc=1, out_pad=4, regime=dict(_RUN, weights='per_unit', nchunk=3, R=4))
_case('run 48->64 sums', (2, 65, 7), 48, 64, 0x1311, stats='sums', regime=dict(_RUN, nchunk=3, stats='fwd', replicas=set(range(8))))
_case('run 24->64 z z_ld+4', (2, 65, 7), 24, 64, 0x1311, stats='z', z_pad=4, bias=False, regime=dict(_RUN, nchunk=3, R=2, stats='bn_z', z_load={'vec'}))
_case('run 8->64 z', (2, 65, 7), 8, 64, 0x1311, stats='z', regime=dict(_RUN, nchunk=1, R=2, stats='bn_z', w_half_instr=True))
_case('run 16->22 z tail', (2, 65, 7), 16, 22, 0x1311, stats='z', out_pad=2, z_pad=2,
      regime={'kernel': 'band', 'nsplit': 2, 'bands_per_wg': 2, 'run_crosses_image': True, 'stores': {'vec', 'tail', 'skip'}, 'z_load': {'vec', 'scalar_tail'}})
_case('run 32->18 z scalar', (2, 65, 7), 32, 18, 0x1311, stats='z', acc=1,
      regime={'kernel': 'band', 'nsplit': 2, 'bands_per_wg': 2, 'stores': {'scalar', 'skip'}, 'z_load': {'scalar_ld'}})
# the same rows at four waves (two workgroups per CU: 128 of them for 130 bands, runs of two) and at twelve
_case('run nw4 32->64 sums', (2, 65, 7), 32, 64, forced(4, 1, 1, 1), stats='sums', acc=1,
      regime={'kernel': 'band', 'NW': 4, 'wgs_per_cu': 2, 'bands_per_wg': 2, 'grid': 260, 'run_crosses_image': True, 'short_last_run': False, 'nchunk': 2})
_case('run nw12 24->64 z', (2, 65, 7), 24, 64, forced(12, 1, 1, 1), stats='z', out_pad=4,
      regime={'kernel': 'band', 'NW': 12, 'R': 2, 'wgs_per_cu': 1, 'bands_per_wg': 3, 'grid': 176, 'run_crosses_image': True, 'short_last_run': True, 'nchunk': 3})
# accumulating into bands with a partial last tile and a short last band -- 33 rows of 7 pixels in bands of 5 (35 pixels: a partial third tile; a last band of
# 3 rows), and 27 rows in bands of 2 dealt in runs of three over five images: a store past a band's pixels or rows would be added twice
_case('run 16->64 th5 acc sums', (3, 33, 7), 16, 64, forced(8, 1, 1, 5), acc=1, stats='sums',
      regime={'kernel': 'band', 'TH': 5, 'nbands': 7, 'total_bands': 21, 'bands_per_wg': 1, 'short_last_band': True, 'last_band_rows': 3, 'partial_tile': True, 'ntile': (3, 2)})
_case('run 32->128 th2 acc', (5, 27, 7), 32, 128, forced(16, 1, 1, 2), acc=1, out_pad=4,
      regime={'kernel': 'band', 'TH': 2, 'nbands': 14, 'total_bands': 70, 'nsplit': 8, 'bands_per_wg': 3, 'short_last_band': True, 'run_crosses_image': True, 'short_last_run': True,
              'partial_tile': True})

# 3. staging: the overflow loop at four waves (six rows of three DMA instructions: 18 against 16 planned), fewer instructions than waves at sixteen,
# rows of one pixel, the 8-byte-aligned 16-byte DMA (in_ld = Cin + 2 at R = 2), in_ld = Cin + 4R
_case('overflow nw4 16->16', (2, 4, 33), 16, 16, forced(4, 1, 4), regime={'kernel': 'band', 'TH': 4, 'th_from': 'H', 'nx': 18, 'overflow_loop': True, 'planned_only': False, 'ipr': 3, 'row_tail': True})
_case('overflow nw4 8->16 R2', (2, 7, 65), 8, 16, forced(4, 1, 8), in_pad=2, regime={'kernel': 'band', 'R': 2, 'TH': 7, 'nx': 27, 'overflow_loop': True, 'ipr': 3, 'row_tail': True})
_case('overflow nw4 32->32 wide', (1, 2, 81), 32, 32, forced(4, 2, 2), regime={'kernel': 'band', 'TH': 1, 'th_from': 'slots', 'nx': 18, 'overflow_loop': True, 'nbands': 2})
_case('idle stagers nw16 16->16', (2, 2, 16), 16, 16, forced(16, 1, 1), regime={'kernel': 'band', 'nx': 4, 'idle_stagers': True, 'row_tail': False, 'tile_spans_rows': False, 'partial_tile': False, 'idle_waves': 14})
_case('busy stagers nw16 16->16', (2, 6, 33), 16, 16, forced(16, 1, 1), acc=1, regime={'kernel': 'band', 'TH': 6, 'th_from': 'H', 'nx': 24, 'idle_stagers': False, 'planned_only': True, 'idle_waves': 3})
_case('in_ld+2 R2 8->16',(2, 5, 7), 8, 16, forced(8, 1, 2), in_pad=2, regime={'kernel': 'band', 'R': 2, 'PPI': 32, 'w_half_instr': True, 'weights': 'once'})
_case('in_ld+2 R2 24->32 W33', (2, 3, 33), 24, 32, forced(12, 1, 3), in_pad=2, acc=1, regime={'kernel': 'band', 'R': 2, 'ipr': 2, 'row_tail': True, 'weights': 'per_unit', 'nchunk': 3})
_case('in+8B R2 8->16', (2, 5, 7), 8, 16, forced(4, 1, 2), in_off=2, regime={'kernel': 'band', 'R': 2})          # every pixel 8 bytes off a 16-byte boundary
_case('in+8B in_ld+2 R2 24->16 run', (2, 9, 33), 24, 16, forced(8, 1, 1, 1), in_off=2, in_pad=2, acc=1, regime={'kernel': 'band', 'R': 2, 'TH': 1, 'total_bands': 18, 'ipr': 2})
_case('in_ld+8 R2 24->16', (2, 3, 17), 24, 16, forced(8, 1, 4), in_pad=8, regime={'kernel': 'band', 'R': 2, 'row_tail': True})
_case('in_ld+16 R4 32->16', (2, 3, 17), 32, 16, forced(8, 1, 4), in_pad=16, bias=False, regime={'kernel': 'band', 'R': 4, 'ipr': 2, 'row_tail': True})
_case('W32 R2 8->16', (2, 3, 32), 8, 16, forced(4, 1, 2), regime={'kernel': 'band', 'R': 2, 'row_tail': False, 'ipr': 1})
_case('W15 R2 24->16', (2, 3, 15), 24, 16, forced(4, 1, 1), regime={'kernel': 'band', 'R': 2, 'row_tail': True, 'TH': 3})
_case('W16 R2 8->16', (2, 3, 16), 8, 16, forced(16, 1, 1), regime={'kernel': 'band', 'R': 2, 'row_tail': True, 'partial_tile': False})
_case('W17 R2 8->32', (2, 3, 17), 8, 32, forced(4, 2, 1), regime={'kernel': 'band', 'R': 2, 'w_half_instr': False})
_case('W33 R2 24->16', (2, 3, 33), 24, 16, forced(8, 1, 2), regime={'kernel': 'band', 'R': 2, 'ipr': 2, 'row_tail': True})
_case('H1 16->16', (3, 1, 21), 16, 16, forced(4, 1, 2), stats='sums', regime={'kernel': 'band', 'H1': True, 'one_band_image': True, 'bands_per_wg': 1})
_case('H1 W1 run 16->16', (300, 1, 1), 16, 16, forced(8, 1, 1), acc=1, regime={'kernel': 'band', 'H1': True, 'total_bands': 300, 'bands_per_wg': 2, 'grid': 150, 'run_crosses_image': True})

# 4. destinations: Cout 6, 18, 24 (tail and skip), out_ld = Cout + 4 / + 1, with the statistics on top
_case('cout6 16->6 out_ld+2', (2, 5, 7), 16, 6, forced(4, 1, 2), out_pad=2, stats='sums', regime={'kernel': 'band', 'stores': {'vec', 'tail', 'skip'}})
_case('cout6 8->6 dense', (2, 5, 7), 8, 6, forced(8, 1, 1), acc=1, regime={'kernel': 'band', 'stores': {'scalar', 'skip'}})
_case('cout18 16->18 out_ld+2 z', (2, 5, 7), 16, 18, forced(4, 2, 2), out_pad=2, stats='z', z_pad=2, regime={'kernel': 'band', 'stores': {'vec', 'tail', 'skip'}, 'z_load': {'vec', 'scalar_tail'}})
_case('cout18 24->18 out_ld+1 acc', (2, 5, 7), 24, 18, forced(12, 1, 3), out_pad=1, acc=1, stats='sums', regime={'kernel': 'band', 'stores': {'scalar', 'skip'}})
_case('cout24 32->24', (2, 5, 7), 32, 24, forced(8, 2, 1), bias=False, stats='z', regime={'kernel': 'band', 'stores': {'vec', 'skip'}, 'z_load': {'vec'}})
_case('cout24 8->24 out_ld+4 acc', (2, 7, 9), 8, 24, forced(4, 1, 1, 3), out_pad=4, acc=1, regime={'kernel': 'band', 'stores': {'vec', 'skip'}, 'nsplit': 2, 'short_last_band': True, 'last_band_rows': 1})
_case('cout16 16->16 z_ld+1', (2, 5, 7), 16, 16, forced(16, 1, 1), stats='z', z_pad=1, regime={'kernel': 'band', 'z_load': {'scalar_ld'}, 'stores': {'vec'}})

# pointers 4 bytes off a 16-byte boundary: `out` (dense Cout % 4 == 0 channels stored as scalars), and bias, bn_z (16-byte loads of any 4-byte-aligned
# address) and bn_coef, of which the kernel asks no alignment
_case('out+4B 16->16 acc', (2, 7, 9), 16, 16, forced(8, 1, 1, 3), acc=1, out_off=1, stats='sums', regime={'kernel': 'band', 'vec_out': False, 'stores': {'scalar'}, 'short_last_band': True})
_case('out+4B 8->32 out_ld+4', (2, 5, 7), 8, 32, forced(4, 2, 2), out_off=1, out_pad=4, regime={'kernel': 'band', 'vec_out': False, 'stores': {'scalar'}})
_case('z+4B bias+4B coef+4B 16->32', (2, 7, 9), 16, 32, forced(4, 2, 1, 3), stats='z', z_off=1, bias_off=1, coef_off=1, regime={'kernel': 'band', 'z_load': {'vec'}, 'stores': {'vec'}})
_case('z+4B z_ld+4 24->22', (2, 5, 7), 24, 22, forced(12, 2, 3), stats='z', z_off=1, z_pad=6, out_pad=2, coef_off=3, regime={'kernel': 'band', 'z_load': {'vec', 'scalar_tail'}})

# 5. fused statistics small enough for the integer sums of squares to stay below 2^24, one per NW (Cin = 8 or 16, 70 pixels)
for _nw, _ci in ((4, 8), (8, 16), (12, 8), (16, 16)):
    _case('exact sums nw%d %d->16' % (_nw, _ci), (2, 5, 7), _ci, 16, forced(_nw, 1, 1), stats='sums', regime={'kernel': 'band', 'NW': _nw, 'stats': 'fwd', 'total_bands': 2, 'replicas': {0, 1}})

# 6. bf16 operands (bit 20): one per NW, two and three chunks, a multi-band run; at R = 2 the bit is ignored
_case('bf16 nw4 16->32', (2, 5, 7), 16, 32, forced(4, 2, 2, bf=1), regime={'kernel': 'band', 'bf': True, 'NW': 4})
_case('bf16 nw8 32->16 acc', (2, 3, 17), 32, 16, forced(8, 1, 4, bf=1), acc=1, out_pad=4, regime={'kernel': 'band', 'bf': True, 'NW': 8, 'nchunk': 2})
_case('bf16 nw12 16->48 sums', (2, 7, 9), 16, 48, forced(12, 3, 3, 3, bf=1), stats='sums', regime={'kernel': 'band', 'bf': True, 'NW': 12})
_case('bf16 nw16 48->16 z', (2, 3, 33), 48, 16, forced(16, 1, 2, bf=1), stats='z', bias=False, regime={'kernel': 'band', 'bf': True, 'NW': 16, 'nchunk': 3})
_case('bf16 run 32->64', (2, 65, 7), 32, 64, 0x1311 | BF16_BIT, regime=dict(_RUN, bf=True, nchunk=2))
_case('bf16 default 16->16', (2, 5, 7), 16, 16, BF16_BIT, regime={'kernel': 'band', 'bf': True, 'forced': False, 'tile': (1, 8)})
_case('bf16 ignored R2 8->16', (2, 5, 7), 8, 16, forced(8, 1, 1, bf=1), regime={'kernel': 'band', 'bf': False, 'R': 2})

# 7. the default (algo 0 and 2): what the search of launch_conv3x3_lds picks.  Few bands against 512 slots: every score is 0 and the first candidate -- the
# largest NT that divides ntile_n with the largest MTW inside the budget -- wins ((4, 4) with two weight units: 84 KiB, one workgroup per CU); from six bands
# on the fill term is above 0 and decides, for (1, 8) at four n-splits and for (1, 1) with one row (2 x 3 x 33) or nine rows (2 x 65 x 7) per band
_case('default 16->16', (2, 5, 7), 16, 16, 0, regime={'kernel': 'band', 'forced': False, 'NW': 4, 'tile': (1, 8), 'TH': 5, 'th_from': 'H', 'wgs_per_cu': 2, 'score': 0})
_case('default 8->32 algo2', (2, 5, 7), 8, 32, 2, acc=1, regime={'kernel': 'band', 'forced': False, 'tile': (2, 8), 'TH': 5, 'wgs_per_cu': 2})
_case('default 32->48', (2, 3, 33), 32, 48, 0, stats='sums', regime={'kernel': 'band', 'forced': False, 'tile': (1, 1), 'TH': 1, 'th_from': 'slots', 'wgs_per_cu': 2, 'score': 300})
_case('default 16->64 algo2', (2, 3, 17), 16, 64, 2, bias=False, regime={'kernel': 'band', 'forced': False, 'tile': (1, 8), 'TH': 3, 'wgs_per_cu': 2, 'score': 138})
_case('default 16->48 one pixel', (1, 1, 1), 16, 48, 0, stats='z', regime={'kernel': 'band', 'forced': False, 'tile': (3, 4), 'TH': 1, 'th_from': 'H', 'score': 0})
_case('default 32->64 one per CU', (1, 3, 17), 32, 64, 2, acc=1, regime={'kernel': 'band', 'forced': False, 'tile': (4, 4), 'TH': 3, 'wgs_per_cu': 1, 'lds_bytes': 85888, 'score': 0})
_case('default 16->16 scored', (2, 65, 7), 16, 16, 0, regime={'kernel': 'band', 'forced': False, 'tile': (1, 1), 'TH': 9, 'th_from': 'slots', 'wgs_per_cu': 2, 'score': 300, 'grid': 16})
# a row of 513 pixels: eight tiles of four waves hold 512, nothing fits and the call falls through to conv_mfma_k
_case('default 8->16 W513 falls through', (1, 1, 513), 8, 16, 0, regime={'kernel': 'mfma', 'fell_through': True, 'forced': False})

# 8. refusals
_case('refused NT does not divide', (2, 5, 7), 16, 48, 0x221, refusal='forced tile: ntile_n % NT')
_case('refused MTW 3 at four waves', (2, 5, 7), 16, 16, 0x213, refusal='forced tile: nothing fits')
_case('refused budget nw8 (4, 8)', (1, 17, 57), 32, 64, 0x348, refusal='forced tile: accumulator budget')
_case('refused budget nw16 (4, 4)', (2, 5, 7), 16, 64, 0x444, refusal='forced tile: accumulator budget')
_case('refused nw12 (3, 2)', (2, 5, 7), 16, 48, 0x732, refusal='forced tile: accumulator budget')
_case('refused force_th', (2, 5, 33), 16, 16, 0x3211, refusal='forced tile: force_th')
_case('refused lds nw8 (1, 8)', (1, 17, 57), 32, 64, 0x318, refusal='forced tile: lds')
_case('refused row too wide', (1, 2, 81), 16, 16, 0x211, refusal='forced tile: row wider than the tile slots')

RUN_CASES = [n for n, c in CASES.items() if not c['refusal']]
REFUSED_CASES = [n for n, c in CASES.items() if c['refusal']]
BAND_CASES = [n for n in RUN_CASES if not n.endswith('falls through')]
FORCED_CASES = [n for n in BAND_CASES if (CASES[n]['algo'] >> 8) & 15]
DEFAULT_CASES = [n for n in BAND_CASES if not (CASES[n]['algo'] >> 8) & 15]


# ---------------------------------------------------------------------------------------------------------------------
# float32 on the CPU, with emulated faults of conv3x3_lds_k
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ('halo_neighbour', 'short_band_halo', 'partial_tile', 'stale_weights', 'second_weight_buffer', 'no_accumulate', 'no_image_wrap')


def operands(pr):
    """(x, Wm) as the matrix pipe sees them: rounded to bf16 (nearest even) under bit 20"""
    if cc.case_regime(pr['case']).get('bf'):
        return cc.bf16_round(pr['x']), cc.bf16_round(pr['Wm'])
    return pr['x'], pr['Wm']


def band_pixels(reg, case):
    """[(b, y0, th)] of every band"""
    return [(b, k * reg['TH'], min(reg['TH'], case['H'] - k * reg['TH'])) for b in range(case['B']) for k in range(reg['nbands'])]


def fault_region(pr, fault):
    """the [B, H, W, Cout] bool mask of the elements a fault moves (None: it does not apply to the case)"""
    c = pr['case']
    reg = cc.case_regime(c)
    B, H, W, C = c['B'], c['H'], c['W'], c['cout']
    m = torch.zeros(B, H, W, C, dtype=torch.bool)
    if fault == 'halo_neighbour':                                    # (every image has a first and a last row)
        m[:, 0], m[:, -1] = True, True
    elif fault == 'short_band_halo':
        if not reg['short_last_band']:
            return None
        m[:, -1] = True
    elif fault == 'partial_tile':
        if not reg['partial_tile']:
            return None
        for b, y0, th in band_pixels(reg, c):
            if (th * W) % 16:
                m[b].view(H * W, C)[y0 * W + (th * W) // 16 * 16:(y0 + th) * W] = True
    elif fault == 'stale_weights':
        if reg['nchunk'] == 1:
            return None
        m[:] = True
    elif fault == 'second_weight_buffer':
        if reg['nchunk'] > 1 or reg['bands_per_wg'] == 1:
            return None
        for lo, hi in reg['runs']:
            for band in range(lo + 1, hi, 2):
                b, y0 = band // reg['nbands'], (band % reg['nbands']) * reg['TH']
                m[b, y0:y0 + reg['TH']] = True
    elif fault == 'no_accumulate':
        if not c['acc']:
            return None
        m[:] = True
    elif fault == 'no_image_wrap':
        if not reg['run_crosses_image']:
            return None
        for lo, hi in reg['runs']:
            for band in range(lo, hi):
                if band // reg['nbands'] != lo // reg['nbands']:
                    b, y0 = band // reg['nbands'], (band % reg['nbands']) * reg['TH']
                    m[b, y0:y0 + reg['TH']] = True
    else:
        raise ValueError(fault)
    return m


def _taps(xpad, Wm, H, W):
    out = torch.zeros(xpad.shape[0], H, W, Wm.shape[2], dtype=xpad.dtype)
    for ky in range(3):
        for kx in range(3):
            out += xpad[:, ky:ky + H, kx:kx + W] @ Wm[ky * 3 + kx]
    return out


def emulate(pr, fault=None):
    """float32: the nine taps added one by one over the zero-padded input.  Faults:
      halo_neighbour   the row above / below an image is the flat neighbour row of the input view -- the last row of the image before, the first of the next,
                       NaN (the guard) outside the view -- instead of rv_zero_piece: the `rowok` select
      short_band_halo  the same for the rows past H of a short last band only
      partial_tile     the partial last tile of a band is not stored
      stale_weights    chunk c is multiplied with the weights of chunk c - 1 (the weight buffer of the unit before)
      second_weight_buffer  one chunk, staged once into weight buffer 0: the odd units of a run read buffer 1, which nothing filled (NaN here) -- the
                       `(nchunk > 1) ? buf : 0` select
      no_accumulate    `accumulate` ignored
      no_image_wrap    the staging cursor does not wrap at H: the bands of a run behind an image boundary are staged from rows past H, i.e. as zeros
    -> out [B, H, W, Cout] float32"""
    c = pr['case']
    reg = cc.case_regime(c)
    B, H, W, Cin = c['B'], c['H'], c['W'], c['cin']
    x, Wm = operands(pr)
    xpad = torch.zeros(B, H + 2, W + 2, Cin)
    xpad[:, 1:H + 1, 1:W + 1] = x
    if fault in ('halo_neighbour', 'short_band_halo'):
        if fault == 'halo_neighbour':
            xpad[0, 0, 1:W + 1] = cc.NAN
            xpad[1:, 0, 1:W + 1] = x[:-1, H - 1]
        xpad[B - 1, H + 1, 1:W + 1] = cc.NAN
        xpad[:B - 1, H + 1, 1:W + 1] = x[1:, 0]
    if fault == 'stale_weights':
        Wm = Wm.roll(4 * reg['R'], 1)
    out = _taps(xpad, Wm, H, W)
    if fault == 'no_image_wrap':
        out = torch.where(fault_region(pr, fault), torch.zeros(()), out)
    if fault == 'second_weight_buffer':
        out = torch.where(fault_region(pr, fault), torch.full((), cc.NAN), out)
    if pr['bias'] is not None:
        out = out + pr['bias']
    start = pr['out0'] if c['acc'] else torch.full_like(out, cc.NAN)  # what the destination holds before the call
    if c['acc'] and fault != 'no_accumulate':
        out = out + pr['out0']
    if fault == 'partial_tile':
        out = torch.where(fault_region(pr, fault), start, out)
    return out


def replica_sums(pr, out, drop=None):
    """the statistics workspace conv3x3_lds_k leaves: workgroup blockIdx (virtual id xcd_remap(blockIdx), band group vid / nsplit, n-split vid % nsplit) adds the
    pixels of its run of bands, for its NT * 16 channels, into replica blockIdx % RV_BN_NREP.  drop: that workgroup's atomics are left out (the emulated fault)."""
    c = pr['case']
    reg = cc.case_regime(c)
    C, W = c['cout'], c['W']
    ws = torch.zeros(RV_BN_NREP * 2 * C + cc.SUMS_GUARD, dtype=torch.float64)
    ws[RV_BN_NREP * 2 * C:] = cc.SUMS_MARK
    v = ws[:RV_BN_NREP * 2 * C].view(RV_BN_NREP, 2, C)
    t1, t2 = cc.stats_terms(pr, out)
    t1, t2 = t1.view(c['B'], c['H'] * W, C), t2.view(c['B'], c['H'] * W, C)
    bands = band_pixels(reg, c)
    for blk in range(reg['grid']):
        if blk == drop:
            continue
        vid = xcd_remap(blk, reg['grid'])
        lo, hi = reg['runs'][vid // reg['nsplit']]
        c0 = (vid % reg['nsplit']) * reg['tile'][0] * 16
        c1 = min(c0 + reg['tile'][0] * 16, C)
        for b, y0, th in bands[lo:hi]:
            v[blk % RV_BN_NREP, 0, c0:c1] += t1[b, y0 * W:(y0 + th) * W, c0:c1].sum(0)
            v[blk % RV_BN_NREP, 1, c0:c1] += t2[b, y0 * W:(y0 + th) * W, c0:c1].sum(0)
    return ws
