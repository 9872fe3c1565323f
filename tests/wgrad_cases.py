"""Case table, launch arithmetic, inputs and references for the weight gradient of csrc/conv.hip: wgrad_mfma_k (fp32 and bf16 operands),
wgrad_wino_k, wgrad_small_k, wgrad_small_sw_k, wgrad_cin1_k, wgrad_reduce_k and wgrad_reduce_table_k behind rv_conv_wgrad, rv_conv_wgrad_seg,
rv_conv_wgrad_deferred, rv_conv_wgrad_deferred_seg and rv_wgrad_reduce_table.

What wgrad_plan, wgrad_sliced, rv_conv_wgrad_workspace_bytes, conv_wgrad_impl and the kernels decide on the host or per workgroup is restated
here in Python (`plan`, `sliced`, `workspace_bytes`, `regime`), and every case carries the regime it is meant to reach.
tests/test_wgrad_cases.py asserts on the CPU that each case lands in its regime, that the cases together reach every regime and every
template instantiation, that the reference equals torch's autograd, that torch's float32 weight gradient meets every derived bound and
that emulated kernel faults miss it; tests/test_wgrad_regimes_gpu.py runs the kernels through the C ABI.

Detection is by construction, as in tests/gemm_cases.py and tests/conv_cases.py.  Every case runs two problems:
  * the INTEGER problem: U, V and the start values from {+-1, +-2, +-3}.  Every partial sum is an integer (the Winograd form: a multiple of
    1/4) below 2^24, so the float32 result is exact in any order -- partial sums, the x-group tree, the reduction tree, the atomics of the
    table, the bf16 operands (exact in bf16) -- and must equal the int64 reference with `==`.  This is what sees a term counted once too few
    or once too often, at every size;
  * the FLOAT problem: magnitudes uniform in [0.5, 1], random sign, against float64 of the same float32 inputs under
        |got - ref| <= 1.01 (N + 2) 2^-24 (sum_p |U||V| + |dw0|)        per element,
    N the number of pixel terms of the element: a sum of N products in ANY order puts at most N - 1 additions, one product rounding and
    one rounding of the final accumulate on the path of a term; 1.01 covers the second-order terms.  The bf16 form is held against float64
    products of the bf16-rounded operands under the same bound (its accumulation is fp32); its bias gradient sums the unrounded V.
    The Winograd form computes dW = G^T [sum_tiles (B^T d B) .* (A y A^T)] G.  A term d_i y_j of the expansion passes through two additions
    of B^T d B (each entry: a sum of two values per direction), two of A y A^T, the product, at most Nt - 1 additions of the sum over the
    Nt tiles (in-wave chain, x-group tree, partial sums, reduction: any order), four roundings of G^T M G (per direction `h = (m1 + m2) / 2`
    and `m0 + h`; the halvings are exact) and the final accumulate: Nt + 10 roundings.  With the absolute transforms
        Wabs = |G^T| [sum_tiles (|B^T| |d| |B|) .* (|A| |y| |A^T|)] |G|         (row sums: |B^T| 2, |A| 1 2 2 1, |G^T| 2 1 2)
    the bound is 1.01 (Nt + 10) 2^-24 (Wabs + |dw0|).
The bounds grow like N^2 and a dropped term does not: in the float problem a single dropped term (>= 0.25) misses the bound by 10x only
while N (N + 2) <= 4e5, i.e. up to some 600 pixel terms (the Winograd form: some 70 tiles).  test_wgrad_cases.py asserts that every kernel
and mode has such a case; the larger grids (the 256-part cases, the 1 056-pixel row that does not fit the Winograd ring, the 4 369-pixel
strips) rest on the integer problem.

U and V live in NaN buffers (guards, skipped channels of u_ld > Ca, the heap between segments); dw and dbias in buffers prefilled with
PAD_BITS, of which everything but the live elements must come back bit-unchanged; the workspace is NaN-filled with a PAD_BITS guard behind it.
"""
import json
import os

import torch
import torch.nn.functional as F

import conv_cases as cc
from conv_cases import GUARD, PAD_BITS, U as EPS, cdiv, err_ratio

TAPS = {0: 9, 1: 1, 2: 4}
GEOM = {0: (3, 3, 1, 1), 1: (1, 1, 1, 0), 2: (2, 2, 2, 0)}          # (KH, KW, S, P)
BF16 = 0x100                                                        # mode bit 8 of rv_conv_wgrad
LDS_MAX = 160 * 1024
WINO_MAXP, WINO_NW = 4, 8                                           # pieces per row and wave planned in registers; waves
TILE_OF = {(8, 16): (1, 1), (16, 32): (1, 2), (24, 8): (2, 1), (32, 24): (2, 2)}       # the channel pairs of the instantiation cases
RV_WS = [(0, 1, 16), (0, 8, 2), (0, 8, 1), (1, 1, 16)]              # wgrad_small_k instantiations: (mode, Ca, Cb)
REDUCE_IMM = [(64, 1), (16, 1), (64, 0), (16, 0), (4, 0)]           # wgrad_reduce_k<EL, V4>
REDUCE_TAB = [(1024, 1), (64, 1), (16, 1), (64, 0), (16, 0), (4, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def plan(taps, B, Hv, Ca, Cb, tune=(0, 0)):
    """mirrors wgrad_plan with the table entry `tune` = (nw, wgs) of rv_conv_wgrad_set_plan ((0, 0): as if there were none)"""
    nrows = B * Hv
    small = Ca * Cb * taps <= 144 and (Ca < 8 or Cb < 8)
    if small:
        return {'small': True, 'TA': 1, 'TB': 1, 'nga': 1, 'ngb': 1, 'rows_per_wave': 0, 'nparts': min(nrows, 4096), 'nw': 0, 'wino': False,
                'units': nrows, 'want': None, 'tie': False}
    best, TA, TB, pads = -1, 1, 1, []
    for ta in (2, 1):
        for tb in (2, 1):
            padded = cdiv(Ca, ta * 16) * ta * cdiv(Cb, tb * 16) * tb
            pads.append(padded)
            if best < 0 or padded < best:                            # ties go to the earlier, i.e. larger, group
                best, TA, TB = padded, ta, tb
    nga, ngb = cdiv(Ca, TA * 16), cdiv(Cb, TB * 16)
    nw, wgs = tune
    total = wgs if wgs > 0 else 256
    wino = bool(nw & 16) and taps == 9 and Hv % 2 == 0
    want = max(total // (nga * ngb), 4)
    units = nrows // 2 if wino else nrows
    rpw = cdiv(units, min(want, units))
    return {'small': False, 'TA': TA, 'TB': TB, 'nga': nga, 'ngb': ngb, 'rows_per_wave': rpw, 'nparts': cdiv(units, rpw), 'nw': nw & 15, 'wino': wino,
            'units': units, 'want': want, 'tie': pads.count(best) > 1}


def sliced(taps, Ca, Cb):
    return taps == 9 and Ca == 1 and Cb > 16 and Cb % 16 == 0


def workspace_bytes(taps, B, Hv, Ca, Cb, tune=(0, 0)):
    if sliced(taps, Ca, Cb):
        Cb = 16
    return plan(taps, B, Hv, Ca, Cb, tune)['nparts'] * (taps * Ca * Cb + Cb) * 4


def plan_key(mode, B, Hv, Ca, Cb):
    """the key of the tuning table a call consults"""
    taps = TAPS[mode & 0xff]
    return (taps, B, Hv, Ca, 16 if sliced(taps, Ca, Cb) else Cb)


def table_prefix(counts):
    """mirrors rv_wgrad_table_finalize -> (exclusive prefixes, total)"""
    out, total = [], 0
    for n in counts:
        out.append(total)
        total += n
    return out, total


def table_lookup(prefix, block):
    """mirrors the bisection of wgrad_reduce_table_k -> entry index"""
    lo, hi = 0, len(prefix) - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if prefix[mid] <= block:
            lo = mid
        else:
            hi = mid - 1
    return lo


def wino_sizes(TA, TB, Wv):
    WT = (Wv + 1) // 2
    WT4 = (WT + 3) & ~3
    ppa, ppb = 64 // (TA * 4), 64 // (TB * 4)
    UPp, VPp = cdiv(2 * WT4 + 2, ppa) * ppa, cdiv(2 * WT4, ppb) * ppb
    lds = (6 * UPp * TA * 16 + 4 * VPp * TB * 16) * 4
    nh = 2 if (TA, TB) == (2, 2) else 1
    nxg = 8 // nh
    fold = nh * (nxg // 2) * (9 * (TA // nh) * TB + TB) * 4 * 64 * 4
    return {'WT': WT, 'WT4': WT4, 'UPp': UPp, 'VPp': VPp, 'lds': max(lds, fold), 'NH': nh, 'NXG': nxg, 'u_pieces': UPp // ppa, 'v_pieces': VPp // ppb,
            'generic_loop': max(UPp // ppa, VPp // ppb) > WINO_MAXP * WINO_NW}


def direct_sizes(mode, TA, TB, nw, Wv, bf):
    KH, _, S, _ = GEOM[mode]
    nslot = KH + 1 if S == 1 else 2 * KH

    def lds_of(Wv4):
        UP = S * (Wv4 - 1) + KH
        return UP, (nslot * UP * TA * 16 + 2 * Wv4 * TB * 16) * 4
    Wv4 = (Wv + 15) & ~15 if bf else (Wv + 3) & ~3
    UP, lds = lds_of(Wv4)
    if bf and lds > 156 * 1024:
        bf, Wv4 = False, (Wv + 3) & ~3
        UP, lds = lds_of(Wv4)
    nh = 2 if (nw == 8 and (TA, TB) == (2, 2)) else 1
    nxg = nw // nh
    fold = nh * (nxg // 2) * (TAPS[mode] * (TA // nh) * TB + TB) * 4 * 64 * 4
    step = 16 if bf else 4
    ksteps = [len(range(xg * step, Wv4, step * nxg)) for xg in range(nxg)]
    return {'bf': bf, 'Wv4': Wv4, 'UP': UP, 'lds': max(lds, fold), 'NH': nh, 'NXG': nxg, 'ksteps': ksteps, 'ksteps_unequal': len({k for k in ksteps if k}) > 1,
            'idle_xgroups': ksteps.count(0), 'last_kstep_partial': Wv % step != 0}


def part_flags(units, rpw, nparts, per_image, per_segment):
    """what the runs [i rpw, min((i + 1) rpw, units)) of rows (row pairs) look like"""
    f, span = set(), 1
    for i in range(nparts):
        r0, r1 = i * rpw, min((i + 1) * rpw, units)
        assert r0 < r1
        if r0 % per_image:
            f.add('mid_image')
        if (r1 - 1) // per_image > r0 // per_image:
            f.add('cross_image')
        if (r1 - 1) // per_segment > r0 // per_segment:
            f.add('cross_segment')
        if r1 - r0 > 1 and (r0 + 1) // per_image == r0 // per_image:
            f.add('prefetch')
        span = max(span, (r1 - 1) // per_image - r0 // per_image + 1)
    if nparts == 1:
        f.add('one_part')
    if units - (nparts - 1) * rpw < rpw:
        f.add('ragged_last')
    return f, span


def reduce_regime(nel, nparts, pstride, ws_off, defer):
    """mirrors the tail of conv_wgrad_impl and the loops of wgrad_reduce_body / wgrad_reduce_body_v4"""
    if cdiv(nel, 64) >= 256 or nparts <= 8:
        el, why = 64, 'nel' if cdiv(nel, 64) >= 256 else 'parts'
    elif cdiv(nel, 16) >= 256 or nparts <= 32:
        el, why = 16, 'nel' if cdiv(nel, 16) >= 256 else 'parts'
    else:
        el, why = 4, 'rest'
    vec4 = int(el >= 16 and nel % 4 == 0 and pstride % 4 == 0 and ws_off % 4 == 0)
    if defer and vec4 and nel >= 8192:
        el, why = 1024, 'deferred'
    PL = 1024 // el if vec4 else 256 // el
    unroll = 4 if vec4 else 2
    entered, tail = False, False
    for pl in range(PL):
        k = pl
        while k + (unroll - 1) * PL < nparts:
            entered = True
            k += unroll * PL
        tail = tail or k < nparts
    return {'nel': nel, 'el': el, 'el_why': why, 'vec4': vec4, 'reduce': (el, vec4), 'reduce_blocks': cdiv(nel, el), 'reduce_unrolled': entered,
            'reduce_tail': tail, 'idle_partial_lanes': PL > nparts}


def regime(mode, B, Hu, Wu, Ca, Hv, Wv, Cb, u_ld=None, v_ld=None, u_off=0, v_off=0, bias=True, tune=(0, 0), nseg=1, defer=False, ws_off=0):
    """What one call does: {'refused': reason} or the regime.  mode may carry BF16; u_off / v_off / ws_off: float offsets from a 16-byte boundary."""
    u_ld = Ca if u_ld is None else u_ld
    v_ld = Cb if v_ld is None else v_ld
    bf, mode = bool(mode & BF16), mode & 0xff
    if not 0 <= mode <= 2:
        return {'refused': 'mode'}
    taps = TAPS[mode]
    if mode == 2 and not (2 * Hv <= Hu <= 2 * Hv + 1 and 2 * Wv <= Wu <= 2 * Wv + 1) or mode != 2 and (Hu, Wu) != (Hv, Wv):
        return {'refused': 'geometry'}
    if not 1 <= nseg <= 4:
        return {'refused': 'segments'}
    if nseg > 1 and (sliced(taps, Ca, Cb) or B % nseg):
        return {'refused': 'no segmented form'}
    if sliced(taps, Ca, Cb):
        if defer:
            return {'refused': 'sliced deferred'}
        r = regime(mode, B, Hu, Wu, 1, Hv, Wv, 16, u_ld, v_ld, u_off, v_off, bias, tune, 1, False, ws_off)
        return r if r['refused'] else dict(r, sliced=Cb // 16)
    pl = plan(taps, B, Hv, Ca, Cb, tune)
    pstride = taps * Ca * Cb + Cb
    reg = {'refused': None, 'sliced': 0, 'mode': mode, 'taps': taps, 'small': pl['small'], 'tile': (pl['TA'], pl['TB']), 'nga': pl['nga'], 'ngb': pl['ngb'],
           'want': pl['want'], 'tie': pl['tie'], 'wino_planned': pl['wino'], 'wino_refused': None, 'fallback': None, 'pstride': pstride,
           'workspace_bytes': pl['nparts'] * pstride * 4}
    nparts, rpw = pl['nparts'], pl['rows_per_wave']
    if pl['small']:
        if nseg > 1:
            return {'refused': 'small segments'}
        u_al, v_al = u_ld % 4 == 0 and u_off % 4 == 0, v_ld % 4 == 0 and v_off % 4 == 0
        strip = None
        if mode == 0 and Ca == 8 and Cb in (1, 2):
            strip = ('sw%d' % Cb, 32, 16) if u_al else None
            reg['fallback'] = None if u_al else ('u_ld' if u_ld % 4 else 'u')
        if mode == 0 and Ca == 1 and Cb == 16:
            strip = ('cin1', 16, 32) if v_al else None
            reg['fallback'] = None if v_al else ('v_ld' if v_ld % 4 else 'v')
        if strip:
            kern, pxw, rows = strip
            nstrip, doubled = cdiv(Wv, pxw), False
            while rows < Hv and B * cdiv(Hv, rows) * nstrip > nparts:
                rows, doubled = rows * 2, True
            nband = cdiv(Hv, rows)
            if B * nband * nstrip <= nparts:
                nparts = B * nband * nstrip
                reg.update(kernel=kern, form=(kern,), rows=rows, rows_doubled=doubled, nstrip=nstrip, nband=nband, last_strip_cols=Wv - (nstrip - 1) * pxw,
                           last_band_rows=Hv - (nband - 1) * rows, h_short=Hv < rows, idle_waves=cdiv(nparts, 4) * 4 - nparts)
            else:
                strip, reg['fallback'] = None, 'tiny'
        if not strip:
            if (mode, Ca, Cb) not in RV_WS:
                return {'refused': 'no small kernel'}
            npix = B * Hv * Wv
            per = cdiv(npix, nparts)
            split_b = Cb >= Ca
            q = min(4, Cb if split_b else Ca)
            cal, cbl = (Ca, q) if split_b else (q, Cb)
            reg.update(kernel='small', form=('small', mode, Ca, Cb), per=per, empty_partials=sum(1 for pw in range(nparts) if pw * per >= npix),
                       ragged_partial=npix % per != 0, idle_waves=cdiv(nparts, 4) * 4 - nparts, uvec=cal % 4 == 0 and u_ld % 4 == 0 and u_off % 4 == 0,
                       vvec=cbl % 4 == 0 and v_ld % 4 == 0 and v_off % 4 == 0)
        reg['parts'] = set()
    else:
        if Ca % 4 or Cb % 4:
            return {'refused': 'channel quads'}
        if u_ld % 4 or v_ld % 4:
            return {'refused': 'strides'}
        if u_off % 4 or v_off % 4:
            return {'refused': 'alignment'}
        TA, TB = pl['TA'], pl['TB']
        wino = pl['wino']
        if wino:
            ws = wino_sizes(TA, TB, Wv)
            why = 'bf16' if (bf and mode == 0) else ('lds' if ws['lds'] > LDS_MAX else None)
            if why:                                                  # planned in row pairs, runs the direct kernel on doubled rows
                wino, reg['wino_refused'] = False, why
                rpw *= 2
                nparts = cdiv(B * Hv, rpw)
        if wino:
            H2 = Hv // 2
            flags, span = part_flags(B * H2, rpw, nparts, H2, (B // nseg) * H2)
            reg.update(ws, kernel='wino', form=('wino', TA, TB), nw=8, nk=[(ws['WT4'] - xg * 4 + 4 * ws['NXG'] - 1) // (4 * ws['NXG']) for xg in range(ws['NXG'])],
                       odd_width=Wv % 2 == 1)
        else:
            nw = pl['nw'] or 8
            ds = direct_sizes(mode, TA, TB, nw, Wv, bf and mode == 0)
            if ds['lds'] > LDS_MAX:
                return {'refused': 'lds'}
            flags, span = part_flags(B * Hv, rpw, nparts, Hv, (B // nseg) * Hv)
            reg.update(ds, kernel='mfma_bf' if ds['bf'] else 'mfma', form=('mfma_bf' if ds['bf'] else 'mfma', mode, TA, TB, nw), nw=nw)
        reg.update(parts=flags, images_spanned=span, padded_a=Ca % (TA * 16) != 0, padded_b=Cb % (TB * 16) != 0, rows_per_wave=rpw)
    if nparts * pstride * 4 > reg['workspace_bytes']:
        return {'refused': 'workspace'}
    reg['nparts'] = nparts
    reg.update(reduce_regime(taps * Ca * Cb + (Cb if bias else 0), nparts, pstride, ws_off, defer))
    return reg


# ---------------------------------------------------------------------------------------------------------------------
# references: the definition in the comment above conv_wgrad_impl
# ---------------------------------------------------------------------------------------------------------------------
def gathered(mode, Uu, Hv, Wv, clamp=()):
    """per tap the U operand on V's grid: yields (tap, sub [B, Hv, Wv, Ca], number of pixels inside per image).  clamp: the sides ('left', 'right', 'top',
    'bottom') whose out-of-image taps read the clamped address instead of zero (the emulated fault)"""
    KH, KW, S, P = GEOM[mode]
    _, Hu, Wu, _ = Uu.shape
    oy, ox = torch.arange(Hv), torch.arange(Wv)
    for ky in range(KH):
        for kx in range(KW):
            iy, ix = oy * S - P + ky, ox * S - P + kx
            oky = ((iy >= 0) | ('top' in clamp)) & ((iy < Hu) | ('bottom' in clamp))
            okx = ((ix >= 0) | ('left' in clamp)) & ((ix < Wu) | ('right' in clamp))
            ok = oky.view(-1, 1) & okx.view(1, -1)
            sub = Uu[:, iy.clamp(0, Hu - 1)][:, :, ix.clamp(0, Wu - 1)] * ok.view(1, Hv, Wv, 1).to(Uu.dtype)
            yield ky * KW + kx, sub, int(ok.sum())


def wgrad_ref(mode, Uu, Vv):
    """Uu [B, Hu, Wu, Ca], Vv [B, Hv, Wv, Cb] (float64 or int64) -> G [taps, Ca, Cb], db [Cb], N [taps] pixel terms per element of a tap"""
    B, Hv, Wv, Cb = Vv.shape
    G = torch.zeros(TAPS[mode], Uu.shape[3], Cb, dtype=Uu.dtype)
    N = torch.zeros(TAPS[mode], dtype=torch.int64)
    for t, sub, n in gathered(mode, Uu, Hv, Wv):
        G[t] = sub.reshape(-1, Uu.shape[3]).t() @ Vv.reshape(-1, Cb)
        N[t] = B * n
    return G, Vv.reshape(-1, Cb).sum(0), N


BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
WA = torch.tensor([[1, 0], [1, 1], [1, -1], [0, -1]], dtype=torch.float64)
WG = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)


def wino_tiles(Uu, Vv):
    """-> d [B, H2, WT, 4, 4, Ca] input patches, y [B, H2, WT, 2, 2, Cb] tiles of V (zeros outside the images)"""
    B, Hv, Wv, Cb = Vv.shape
    H2, WT = Hv // 2, (Wv + 1) // 2
    up = F.pad(Uu.permute(0, 3, 1, 2), (1, 2 * WT - Wv + 1, 1, 1))
    d = up.unfold(2, 4, 2).unfold(3, 4, 2).permute(0, 2, 3, 4, 5, 1)
    vp = F.pad(Vv.permute(0, 3, 1, 2), (0, 2 * WT - Wv))
    y = vp.unfold(2, 2, 2).unfold(3, 2, 2).permute(0, 2, 3, 4, 5, 1)
    return d, y


def wino_wgrad(Uu, Vv, absolute=False):
    """the Winograd F(3x3, 2x2) weight gradient in the dtype of the operands (float32: the emulation; absolute: Wabs of the bound, float64)"""
    dt = Uu.dtype
    bt, wa, wg = (m.abs() if absolute else m for m in (BT, WA, WG))
    bt, wa, wg = bt.to(dt), wa.to(dt), wg.to(dt)
    d, y = wino_tiles(Uu.abs() if absolute else Uu, Vv.abs() if absolute else Vv)
    P = torch.einsum('ik,bhwkla->bhwila', bt, d)
    P = torch.einsum('jl,bhwila->bhwija', bt, P)
    Q = torch.einsum('ik,bhwklc->bhwilc', wa, y)
    Q = torch.einsum('jl,bhwilc->bhwijc', wa, Q)
    M = torch.einsum('bhwija,bhwijc->ijac', P, Q)
    T = torch.einsum('ik,ijac->kjac', wg, M)
    return torch.einsum('jl,kjac->klac', wg, T).reshape(9, Uu.shape[3], Vv.shape[3])


def torch_wgrad(mode, Uu, Vv):
    """the same through torch autograd of F.conv2d, in the dtype of the operands -> G [taps, Ca, Cb], db [Cb]"""
    KH, KW, S, P = GEOM[mode]
    Ca, Cb = Uu.shape[3], Vv.shape[3]
    w = torch.zeros(Cb, Ca, KH, KW, dtype=Uu.dtype, requires_grad=True)
    b = torch.zeros(Cb, dtype=Uu.dtype, requires_grad=True)
    out = F.conv2d(Uu.permute(0, 3, 1, 2), w, b, stride=S, padding=P)
    (out * Vv.permute(0, 3, 1, 2)).sum().backward()
    return w.grad.permute(2, 3, 1, 0).reshape(KH * KW, Ca, Cb), b.grad


# ---------------------------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}
LAYOUTS = ('c', 't', 'gap')        # 'c': dw[b][a][tap] (Conv2d; with taps = 4 also the up conv's dWt[ci][co][tap]), 't': dw[a][b][taps-1-tap] (ConvTranspose2d 3x3)


def layout_of(case):
    """-> (s_a, s_b, flip, floats spanned)"""
    taps, Ca, Cb = TAPS[case['mode']], case['Ca'], case['Cb']
    if case['layout'] == 'c':
        s_a, s_b, flip = taps, Ca * taps, 0
    elif case['layout'] == 't':
        s_a, s_b, flip = Cb * taps, taps, 1
    else:
        s_a, s_b, flip = taps + 2, Ca * (taps + 2) + 3, 0             # gaps behind every tap run and every row
    return s_a, s_b, flip, (Ca - 1) * s_a + (Cb - 1) * s_b + taps


def _case(name, mode, B, Hv, Wv, Ca, Cb, bf=False, up=(0, 0), tune=(0, 0), u_pad=0, v_pad=0, u_off=0, v_off=0, bias=True, acc=0, layout='c', nseg=1,
          defer=False, ws_off=0, refusal=None, regime=None):
    """B: all images (nseg segments of B / nseg).  up: mode 2, Hu = 2 Hv + up[0], Wu = 2 Wv + up[1].  u_pad / v_pad: floats of padding per pixel; u_off / v_off /
    ws_off: float offsets of U / V / the workspace from a 16-byte boundary.  tune: the (nw, wgs) given to rv_conv_wgrad_set_plan."""
    assert name not in CASES, name
    Hu, Wu = (2 * Hv + up[0], 2 * Wv + up[1]) if mode == 2 else (Hv, Wv)
    CASES[name] = {'name': name, 'seed': len(CASES) + 1, 'mode': mode, 'bf': bf, 'B': B, 'Hu': Hu, 'Wu': Wu, 'Hv': Hv, 'Wv': Wv, 'Ca': Ca, 'Cb': Cb, 'tune': tune,
                   'u_pad': u_pad, 'v_pad': v_pad, 'u_off': u_off, 'v_off': v_off, 'bias': bias, 'acc': acc, 'layout': layout, 'nseg': nseg, 'defer': defer,
                   'ws_off': ws_off, 'refusal': refusal, 'regime': regime or {}}


def case_regime(case, **kw):
    c = dict(case, **kw)
    return regime(c['mode'] | (BF16 if c['bf'] else 0), c['B'], c['Hu'], c['Wu'], c['Ca'], c['Hv'], c['Wv'], c['Cb'], c['Ca'] + c['u_pad'], c['Cb'] + c['v_pad'],
                  c['u_off'], c['v_off'], c['bias'], c['tune'], c['nseg'], c['defer'], c['ws_off'])


def case_key(case):
    return plan_key(case['mode'], case['B'], case['Hv'], case['Ca'], case['Cb'])


# 1. every instantiation of the MFMA kernels on B = 2, Hv = 6, Wv = 5 (60 pixels, 12 rows: units < want, one row per workgroup); the options rotate
_VARIANTS = [{}, {'acc': 1, 'layout': 't'}, {'bias': False, 'u_pad': 4, 'v_pad': 8}, {'layout': 'gap', 'acc': 1, 'bias': False}, {'u_pad': 4, 'v_pad': 8, 'layout': 't'},
             {'ws_off': 1}, {'defer': True, 'acc': 1}, {'defer': True, 'layout': 'gap', 'v_pad': 8}]
_UPS = [(0, 0), (0, 1), (1, 0), (1, 1)]
_rr = 0
for _m in (0, 1, 2):
    for (_ca, _cb), _tile in TILE_OF.items():
        for _nw in (4, 8):
            _kw = dict(_VARIANTS[_rr % len(_VARIANTS)])
            _up = _UPS[_rr % 4] if _m == 2 else (0, 0)
            _rr += 1
            _case('mfma m%d %d->%d nw%d' % (_m, _ca, _cb, _nw), _m, 2, 6, 5, _ca, _cb, tune=(_nw, 0), up=_up, **_kw,
                  regime={'kernel': 'mfma', 'form': ('mfma', _m, _tile[0], _tile[1], _nw), 'nparts': 12, 'rows_per_wave': 1, 'NXG': _nw // (2 if _nw == 8 and _tile == (2, 2) else 1)})
for (_ca, _cb), _tile in TILE_OF.items():
    _kw = dict(_VARIANTS[_rr % len(_VARIANTS)])
    _rr += 1
    _case('wino %d->%d' % (_ca, _cb), 0, 2, 6, 5, _ca, _cb, tune=(24, 0), **_kw,
          regime={'kernel': 'wino', 'form': ('wino',) + _tile, 'nparts': 6, 'WT4': 4, 'odd_width': True, 'u_pieces': 1 if _tile[0] == 1 else 2})
    for _nw in (4, 8):
        _kw = dict(_VARIANTS[_rr % len(_VARIANTS)])
        _rr += 1
        _case('bf16 %d->%d nw%d' % (_ca, _cb, _nw), 0, 2, 6, 5, _ca, _cb, bf=True, tune=(_nw, 0), **_kw,
              regime={'kernel': 'mfma_bf', 'form': ('mfma_bf', 0) + _tile + (_nw,), 'Wv4': 16, 'last_kstep_partial': True})

# 2. channel groups: 48 = 3 x 16 (not 2 x 32), nine groups; padded last groups (36 = 2 x 16 + 4, 40 = 2 x 16 + 8, 20 of 32, 12 of 16); the tie rule (20 and 24:
# 2 x 16 = 1 x 32 -> the larger group); the bias is summed by the a-group 0 only
_case('chan 48->48 m0', 0, 2, 35, 2, 48, 48, tune=(8, 4096), regime={'kernel': 'mfma', 'tile': (1, 1), 'nga': 3, 'ngb': 3, 'want': 455, 'nparts': 70, 'reduce': (64, 1), 'el_why': 'nel',
                                                                    'reduce_unrolled': True, 'reduce_tail': True})     # 70 partials: the unrolled loop of the 16-byte body and its tail
_case('chan 48->48 m0 deferred', 0, 2, 35, 2, 48, 48, tune=(4, 4096), defer=True, acc=1, layout='t', regime={'kernel': 'mfma', 'reduce': (1024, 1)})
_case('chan 36->40 m1', 1, 2, 6, 5, 36, 40, tune=(8, 0), acc=1, u_pad=4, regime={'kernel': 'mfma', 'tile': (1, 1), 'nga': 3, 'ngb': 3, 'padded_a': True, 'padded_b': True})
_case('chan 20->12 m2', 2, 2, 6, 5, 20, 12, tune=(8, 0), up=(1, 1), regime={'kernel': 'mfma', 'tile': (2, 1), 'tie': True, 'padded_a': True, 'padded_b': True})
_case('chan 32->48 m0 wino', 0, 2, 6, 5, 32, 48, tune=(24, 0), layout='t', regime={'kernel': 'wino', 'tile': (2, 1), 'nga': 1, 'ngb': 3})
_case('chan 32->48 m0 bf16', 0, 2, 6, 5, 32, 48, bf=True, tune=(4, 0), acc=1, regime={'kernel': 'mfma_bf', 'tile': (2, 1), 'ngb': 3})

# 3. the row partition (8 -> 16 unless the want has to be small: with nine channel groups and wgs = 32 a launch wants 4 workgroups)
_case('part one', 0, 1, 1, 3, 8, 16, tune=(8, 0), regime={'kernel': 'mfma', 'nparts': 1, 'parts': {'one_part'}, 'reduce': (64, 1), 'el_why': 'parts'})
_case('part one deferred', 0, 1, 1, 3, 8, 16, tune=(4, 0), defer=True, regime={'kernel': 'mfma', 'nparts': 1, 'reduce': (64, 1)})
for _nw, _kern in ((8, 'mfma'), (4, 'mfma'), (24, 'mfma')):          # 45 rows in runs of two: ragged, mid-image, across the image boundary; nw = 24 with an odd Hv plans in rows
    _case('part 3x15 wgs32 nw%d' % _nw, 0, 3, 15, 4, 8, 16, tune=(_nw, 32), acc=_nw == 4,
          regime={'kernel': _kern, 'nparts': 23, 'rows_per_wave': 2, 'parts': {'mid_image', 'cross_image', 'ragged_last', 'prefetch'}, 'wino_planned': False, 'nw': 4 if _nw == 4 else 8})
_case('part 9x1 three images', 0, 9, 1, 3, 36, 40, tune=(8, 32), regime={'kernel': 'mfma', 'want': 4, 'nparts': 3, 'rows_per_wave': 3, 'images_spanned': 3})
_case('part 9x2 three images', 0, 9, 2, 3, 36, 40, tune=(4, 32), acc=1, regime={'kernel': 'mfma', 'nparts': 4, 'rows_per_wave': 5, 'images_spanned': 3, 'parts': {'mid_image', 'cross_image', 'ragged_last', 'prefetch'}})
_case('part 9x2 three images wino', 0, 9, 2, 3, 36, 40, tune=(24, 32), regime={'kernel': 'wino', 'nparts': 3, 'rows_per_wave': 3, 'images_spanned': 3})
_case('part 256', 0, 2, 128, 4, 8, 16, tune=(8, 0), regime={'kernel': 'mfma', 'nparts': 256, 'rows_per_wave': 1, 'reduce': (4, 0), 'reduce_unrolled': True})     # 1 024 px: the integer problem carries it
_case('part 256 deferred', 0, 2, 128, 4, 8, 16, tune=(4, 0), defer=True, acc=1, regime={'kernel': 'mfma', 'nparts': 256, 'reduce': (4, 0)})
_case('part wgs4096', 0, 2, 130, 4, 8, 16, tune=(8, 4096), regime={'kernel': 'mfma', 'want': 4096, 'nparts': 260, 'rows_per_wave': 1})
_case('part wgs32', 0, 2, 130, 4, 8, 16, tune=(4, 32), regime={'kernel': 'mfma', 'want': 32, 'nparts': 29, 'rows_per_wave': 9, 'parts': {'mid_image', 'cross_image', 'ragged_last', 'prefetch'}})
_case('part wgs32 wino', 0, 2, 130, 4, 8, 16, tune=(24, 32), layout='t', regime={'kernel': 'wino', 'nparts': 26, 'rows_per_wave': 5, 'parts': {'mid_image', 'prefetch'}})
_case('part default 130', 0, 2, 130, 4, 8, 16, tune=(0, 0), regime={'kernel': 'mfma', 'nparts': 130, 'rows_per_wave': 2, 'nw': 8})

# 4. widths: 1, 3, 4, 37 (5: above); 37 -> 10 k-steps over 8 (4) x groups: unequal; the bf16 form above 16 * NXG pixels
for _w in (1, 3, 4, 37):
    for _m in (0, 1, 2):
        _case('width %d m%d' % (_w, _m), _m, 2, 6, _w, 8, 16, tune=(8 if _w != 3 else 4, 0), up=_UPS[_w % 4], acc=_w == 4,
              regime={'kernel': 'mfma', 'Wv4': (_w + 3) & ~3, 'last_kstep_partial': _w != 4, 'ksteps_unequal': _w == 37, 'idle_xgroups': {1: 7, 3: 3, 4: 7, 37: 0}[_w]})
_case('width 37 wino', 0, 2, 6, 37, 8, 16, tune=(24, 0), u_pad=4, v_pad=8, bias=False, regime={'kernel': 'wino', 'WT4': 20, 'u_pieces': 3, 'v_pieces': 3, 'nk': [1, 1, 1, 1, 1, 0, 0, 0]})
_case('width 8 wino', 0, 2, 6, 8, 8, 16, tune=(24, 0), acc=1, regime={'kernel': 'wino', 'odd_width': False, 'u_pieces': 1, 'v_pieces': 1})
_case('width 37 wino 32->24', 0, 2, 6, 37, 32, 24, tune=(24, 0), layout='gap', u_pad=4, regime={'kernel': 'wino', 'u_pieces': 6, 'NXG': 4, 'nk': [2, 1, 1, 1]})
_case('width 70 bf16 nw4', 0, 2, 6, 70, 8, 16, bf=True, tune=(4, 0), regime={'kernel': 'mfma_bf', 'Wv4': 80, 'NXG': 4, 'ksteps': [2, 1, 1, 1], 'ksteps_unequal': True})
_case('width 133 bf16 nw8', 0, 2, 6, 133, 8, 16, bf=True, tune=(8, 0), regime={'kernel': 'mfma_bf', 'Wv4': 144, 'ksteps': [2, 1, 1, 1, 1, 1, 1, 1]})

# 5. the Winograd form: Hv 2 (above), 4, 6; refused by the LDS (a 132-pixel row of 32 -> 32 channels: 176 KiB of ring) and by the bf16 bit -- direct on doubled rows
_case('wino Hv4 16->32', 0, 2, 4, 6, 16, 32, tune=(24, 0), acc=1, regime={'kernel': 'wino', 'nparts': 4, 'odd_width': False})
_case('wino lds 32->32 W132', 0, 2, 4, 132, 32, 32, tune=(24, 0), regime={'kernel': 'mfma', 'wino_planned': True, 'wino_refused': 'lds', 'rows_per_wave': 2, 'nparts': 4, 'nw': 8})
_case('wino bf16 3x14', 0, 3, 14, 5, 8, 16, bf=True, tune=(24, 32), regime={'kernel': 'mfma_bf', 'wino_planned': True, 'wino_refused': 'bf16', 'rows_per_wave': 2, 'nparts': 21})
_case('bf16 3x14 wgs32', 0, 3, 14, 5, 8, 16, bf=True, tune=(8, 32), regime={'kernel': 'mfma_bf', 'wino_planned': False, 'rows_per_wave': 2, 'nparts': 21})

# 6. the small-channel kernels.  Strips of 32 (8 -> 1, 8 -> 2) / 16 (1 -> 16) columns, bands of 16 / 32 rows
_case('sw1 big', 0, 2, 17, 33, 8, 1, regime={'kernel': 'sw1', 'nstrip': 2, 'nband': 2, 'last_strip_cols': 1, 'last_band_rows': 1, 'nparts': 8, 'reduce': (64, 0), 'el_why': 'parts'})
_case('sw1 big deferred', 0, 2, 17, 33, 8, 1, defer=True, acc=1, u_pad=4, regime={'kernel': 'sw1', 'nparts': 8, 'reduce': (64, 0)})
_case('sw1 fallback u+4B', 0, 2, 17, 33, 8, 1, u_off=1, acc=1, regime={'kernel': 'small', 'form': ('small', 0, 8, 1), 'fallback': 'u', 'uvec': False, 'nparts': 34, 'per': 33, 'reduce': (4, 0), 'idle_waves': 2})
_case('sw1 tiny', 0, 1, 1, 33, 8, 1, bias=False, regime={'kernel': 'small', 'fallback': 'tiny', 'uvec': True, 'nparts': 1})
_case('sw1 1x20', 0, 1, 1, 20, 8, 1, layout='t', bias=False, regime={'kernel': 'sw1', 'nparts': 1, 'h_short': True, 'last_strip_cols': 20})           # (small enough for the float problem to see one term)
_case('sw2 17x20', 0, 1, 17, 20, 8, 2, bias=False, regime={'kernel': 'sw2', 'nparts': 2, 'nband': 2, 'last_band_rows': 1})
_case('small 1x1 1->16 W5', 1, 2, 17, 5, 1, 16, layout='gap', regime={'kernel': 'small', 'per': 5, 'nparts': 34})
_case('sw2 doubled', 0, 1, 17, 257, 8, 2, regime={'kernel': 'sw2', 'rows': 32, 'rows_doubled': True, 'nstrip': 9, 'nband': 1, 'last_strip_cols': 1, 'h_short': True, 'nparts': 9, 'idle_waves': 3})   # 4 369 px: a 17-row image of nine strips
_case('sw2 3 strips', 0, 1, 17, 65, 8, 2, layout='t', v_pad=3, regime={'kernel': 'sw2', 'rows': 16, 'nstrip': 3, 'nband': 2, 'nparts': 6, 'idle_waves': 2})
_case('sw2 fallback u_ld+1', 0, 1, 17, 65, 8, 2, u_pad=1, regime={'kernel': 'small', 'form': ('small', 0, 8, 2), 'fallback': 'u_ld', 'nparts': 17, 'reduce': (16, 0)})
_case('sw2 12 parts', 0, 3, 17, 33, 8, 2, acc=1, layout='gap', regime={'kernel': 'sw2', 'nparts': 12, 'reduce': (16, 0), 'el_why': 'parts'})
_case('sw2 12 parts deferred', 0, 3, 17, 33, 8, 2, defer=True, bias=False, regime={'kernel': 'sw2', 'nparts': 12, 'reduce': (16, 0)})
_case('cin1 big', 0, 2, 33, 17, 1, 16, regime={'kernel': 'cin1', 'nstrip': 2, 'nband': 2, 'last_strip_cols': 1, 'last_band_rows': 1, 'nparts': 8, 'reduce': (64, 1)})
_case('cin1 big v_ld+8 u_ld+1', 0, 2, 33, 17, 1, 16, v_pad=8, u_pad=1, acc=1, bias=False, regime={'kernel': 'cin1', 'nparts': 8})
_case('cin1 H5', 0, 1, 5, 20, 1, 16, layout='t', regime={'kernel': 'cin1', 'h_short': True, 'nstrip': 2, 'last_strip_cols': 4, 'nparts': 2, 'idle_waves': 2})
_case('cin1 doubled', 0, 1, 33, 257, 1, 16, regime={'kernel': 'cin1', 'rows': 64, 'rows_doubled': True, 'nstrip': 17, 'nband': 1, 'nparts': 17, 'reduce': (16, 1)})                       # 8 481 px
_case('cin1 fallback v+4B', 0, 2, 33, 17, 1, 16, v_off=1, regime={'kernel': 'small', 'form': ('small', 0, 1, 16), 'fallback': 'v', 'vvec': False, 'nparts': 66, 'reduce': (4, 0)})
_case('cin1 fallback v_ld+1', 0, 1, 5, 20, 1, 16, v_pad=1, acc=1, regime={'kernel': 'small', 'fallback': 'v_ld', 'vvec': False, 'nparts': 5})
_case('cin1 tiny', 0, 1, 1, 17, 1, 16, regime={'kernel': 'small', 'fallback': 'tiny', 'vvec': True, 'nparts': 1})
_case('small 1x1 1->16', 1, 2, 17, 33, 1, 16, regime={'kernel': 'small', 'form': ('small', 1, 1, 16), 'vvec': True, 'nparts': 34, 'per': 33, 'idle_waves': 2})
_case('small 1x1 1->16 v_ld+1 acc', 1, 2, 17, 33, 1, 16, v_pad=1, acc=1, bias=False, u_pad=2, regime={'kernel': 'small', 'vvec': False})
_case('small 1x1 empty partials', 1, 1, 4097, 1, 1, 16, regime={'kernel': 'small', 'nparts': 4096, 'per': 2, 'empty_partials': 2047, 'ragged_partial': True})   # 4 097 rows: the cap of 4 096 partials
_case('sliced 1->48', 0, 1, 33, 17, 1, 48, acc=1, regime={'kernel': 'cin1', 'sliced': 3, 'nparts': 4})
_case('sliced 1->32 v_ld+1', 0, 1, 33, 17, 1, 32, v_pad=1, layout='t', regime={'kernel': 'small', 'sliced': 2, 'fallback': 'v_ld'})

# 7. segments, scattered over a heap in descending address order
_case('seg2x2 wino 16->32', 0, 4, 4, 6, 16, 32, tune=(24, 0), nseg=2, regime={'kernel': 'wino', 'nparts': 8})
_case('seg3x1 m1 24->8', 1, 3, 5, 5, 24, 8, tune=(8, 0), nseg=3, acc=1, u_pad=4, regime={'kernel': 'mfma', 'nparts': 15})
_case('seg3x1 m0 36->40 crossing', 0, 3, 5, 3, 36, 40, tune=(4, 32), nseg=3, regime={'kernel': 'mfma', 'rows_per_wave': 4, 'nparts': 4, 'parts': {'mid_image', 'cross_image', 'cross_segment', 'ragged_last', 'prefetch'}})
_case('seg4x2 m2 32->24', 2, 8, 3, 4, 32, 24, tune=(8, 0), nseg=4, up=(1, 0), layout='c', regime={'kernel': 'mfma', 'nparts': 24})
_case('seg3x1 wino 36->40 crossing', 0, 3, 10, 3, 36, 40, tune=(24, 32), nseg=3, acc=1, regime={'kernel': 'wino', 'rows_per_wave': 4, 'nparts': 4, 'parts': {'mid_image', 'cross_image', 'cross_segment', 'ragged_last', 'prefetch'}})
_case('seg2x2 wino deferred', 0, 4, 4, 6, 16, 32, tune=(24, 0), nseg=2, defer=True, acc=1, layout='t', regime={'kernel': 'wino'})
_case('seg4x2 m2 deferred', 2, 8, 3, 4, 32, 24, tune=(4, 0), nseg=4, up=(0, 1), defer=True, regime={'kernel': 'mfma'})
_case('seg2x2 bf16', 0, 4, 4, 6, 16, 32, bf=True, tune=(8, 0), nseg=2, regime={'kernel': 'mfma_bf'})

# 8. refusals that are cases (the others: test_wgrad_refusals of the GPU file)
_case('refused 2->8 m0', 0, 1, 4, 4, 2, 8, refusal='no small kernel')
_case('refused 18->12 quads', 1, 1, 4, 4, 18, 12, u_pad=2, refusal='channel quads')
_case('refused u_ld+2', 0, 1, 4, 4, 8, 16, u_pad=2, refusal='strides')
_case('refused v+4B', 1, 1, 4, 4, 8, 16, v_off=1, refusal='alignment')
_case('refused seg small', 0, 2, 17, 33, 8, 1, nseg=2, refusal='small segments')
_case('refused seg sliced', 0, 2, 33, 17, 1, 48, nseg=2, refusal='no segmented form')
_case('refused deferred sliced', 0, 1, 33, 17, 1, 48, defer=True, refusal='sliced deferred')

RUN_CASES = [n for n, c in CASES.items() if not c['refusal']]
REFUSED_CASES = [n for n, c in CASES.items() if c['refusal']]
# the deferred table of the GPU test: el 4, 16 (16-byte loads), 64 (16-byte loads), 1 024, 64 and 16 (scalar), and the third entry once more onto the same destination
TABLE_CASES = ['part 256 deferred', 'mfma m0 32->24 nw4', 'part one deferred', 'chan 48->48 m0 deferred', 'sw1 big deferred', 'sw2 12 parts deferred', 'part one deferred']
ENTRY_BYTES, ENTRY_BLOCK0_AT, ENTRY_EL_AT, ENTRY_VEC4_AT = 96, 80, 88, 92          # sizeof(WreduceEntry) and the offsets of block0, el, vec4


# ---------------------------------------------------------------------------------------------------------------------
# inputs (CPU, seeded per case, cached, never modified by the tests)
# ---------------------------------------------------------------------------------------------------------------------
_problems = {}


def problem(case, kind):
    """One problem of a case: the logical tensors Uu [B, Hu, Wu, Ca], Vv [B, Hv, Wv, Cb], dw0 [taps, Ca, Cb], db0 [Cb] and the flat host buffers they live in.
    Segments sit in one heap each for U and V, segment s at float offset u_at[s] / v_at[s], the LAST segment first."""
    key = (case['name'], kind)
    if key in _problems:
        return _problems[key]
    c = case
    B, Hu, Wu, Hv, Wv, Ca, Cb, nseg = c['B'], c['Hu'], c['Wu'], c['Hv'], c['Wv'], c['Ca'], c['Cb'], c['nseg']
    taps = TAPS[c['mode']]
    g = cc._gen(c['seed'], kind == 'int', 9)
    pr = {'case': c, 'kind': kind, 'u_ld': Ca + c['u_pad'], 'v_ld': Cb + c['v_pad']}
    pr['Uu'], pr['Vv'] = cc._draw(g, kind, B, Hu, Wu, Ca), cc._draw(g, kind, B, Hv, Wv, Cb)
    pr['dw0'] = cc._draw(g, kind, taps, Ca, Cb) if c['acc'] else None
    pr['db0'] = cc._draw(g, kind, Cb) if c['acc'] else None
    Bseg = B // nseg
    for nm, t, H, W, C, ld, off in (('u', pr['Uu'], Hu, Wu, Ca, pr['u_ld'], c['u_off']), ('v', pr['Vv'], Hv, Wv, Cb, pr['v_ld'], c['v_off'])):
        seg = Bseg * H * W * ld
        seg4 = (seg + 3) & ~3
        at = [GUARD + off + (nseg - 1 - s) * (seg4 + GUARD) for s in range(nseg)]
        buf = cc._nan_buffer(GUARD + off + nseg * (seg4 + GUARD))
        for s in range(nseg):
            cc.nhwc_view(buf, at[s], Bseg, H, W, C, ld).copy_(t[s * Bseg:(s + 1) * Bseg])
        pr[nm + '_buf'], pr[nm + '_at'] = buf, at
    s_a, s_b, flip, span = layout_of(c)
    pr['layout'] = (s_a, s_b, flip)
    t_, a_, b_ = torch.arange(taps).view(-1, 1, 1), torch.arange(Ca).view(1, -1, 1), torch.arange(Cb).view(1, 1, -1)
    pr['dw_idx'] = GUARD + a_ * s_a + b_ * s_b + ((taps - 1 - t_) if flip else t_)
    assert pr['dw_idx'].unique().numel() == taps * Ca * Cb
    pr['dw_buf'] = cc._pad_buffer(GUARD + span + GUARD)
    pr['db_buf'] = cc._pad_buffer(GUARD + Cb + GUARD)
    if c['acc'] or c['defer']:                                        # the deferred form ADDS: onto the start values, or onto zeros
        pr['dw_buf'][pr['dw_idx'].reshape(-1)] = (pr['dw0'] if c['acc'] else torch.zeros(taps, Ca, Cb)).reshape(-1)
        if c['bias']:
            pr['db_buf'][GUARD:GUARD + Cb] = pr['db0'] if c['acc'] else torch.zeros(Cb)
    _problems[key] = pr
    return pr


def live(pr, dw_buf, db_buf):
    """-> G [taps, Ca, Cb], db [Cb] read out of the destination buffers"""
    return dw_buf[pr['dw_idx'].reshape(-1)].view(pr['dw_idx'].shape), db_buf[GUARD:GUARD + pr['case']['Cb']]


def padding_intact(pr, dw_buf, db_buf):
    """every float of the destination buffers outside the live elements still holds PAD_BITS; without a bias the whole dbias buffer does"""
    w = dw_buf.detach().cpu().clone().view(torch.int32)
    w[pr['dw_idx'].reshape(-1)] = PAD_BITS
    b = db_buf.detach().cpu().clone().view(torch.int32)
    if pr['case']['bias']:
        b[GUARD:GUARD + pr['case']['Cb']] = PAD_BITS
    return bool((w == PAD_BITS).all().item()) and bool((b == PAD_BITS).all().item())


# ---------------------------------------------------------------------------------------------------------------------
# references and comparisons
# ---------------------------------------------------------------------------------------------------------------------
_refs = {}


def bf16_round(t):
    return t.bfloat16().to(t.dtype)


def reference(pr):
    """-> {'G', 'db' float64 (the integer problem: computed in int64), 'G_bound', 'db_bound', 'N'}"""
    key = (pr['case']['name'], pr['kind'])
    if key in _refs:
        return _refs[key]
    c = pr['case']
    reg = case_regime(c)
    dt = torch.int64 if pr['kind'] == 'int' else torch.float64
    Uu, Vv = pr['Uu'], pr['Vv']
    Uo, Vo = (bf16_round(Uu), bf16_round(Vv)) if reg['kernel'] == 'mfma_bf' else (Uu, Vv)
    G, _, N = wgrad_ref(c['mode'], Uo.to(dt), Vo.to(dt))
    db = Vv.to(dt).reshape(-1, c['Cb']).sum(0)                       # (the bf16 kernel sums the unrounded V)
    mag, dbmag, _ = wgrad_ref(c['mode'], Uo.double().abs(), Vo.double().abs())
    if reg['kernel'] == 'wino':
        mag = wino_wgrad(Uo.double(), Vo.double(), absolute=True)
        nterm = torch.full((9, 1, 1), float(c['B'] * (c['Hv'] // 2) * reg['WT'] + 10))
    else:
        nterm = (N + 2).double().view(-1, 1, 1)
    G, db = G.double(), db.double()
    if c['acc']:
        G, db = G + pr['dw0'].double(), db + pr['db0'].double()
        mag, dbmag = mag + pr['dw0'].double().abs(), dbmag + pr['db0'].double().abs()
    ref = {'G': G, 'db': db, 'N': N, 'G_bound': 1.01 * nterm * EPS * mag, 'db_bound': 1.01 * (c['B'] * c['Hv'] * c['Wv'] + 2) * EPS * dbmag}
    _refs[key] = ref
    return ref


def compare(pr, G, db):
    """-> (ratio of G, ratio of db) against reference(pr); <= 1 passes.  The integer problem is exact: its bound is 0."""
    ref = reference(pr)
    zero = pr['kind'] == 'int'
    rg = err_ratio(G, ref['G'], torch.zeros_like(ref['G_bound']) if zero else ref['G_bound'])
    rb = err_ratio(db, ref['db'], torch.zeros_like(ref['db_bound']) if zero else ref['db_bound']) if pr['case']['bias'] else 0.0
    return rg, rb


def dropped_term_margin(pr):
    """the smallest single term of the float problem (0.5 * 0.5) over the largest bound of the case: >= 10 means one dropped term fails by 10x"""
    ref = reference(pr)
    return 0.25 / max(ref['G_bound'].max().item(), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# float32 on the CPU along the partition of the mirror, with emulated kernel faults
# ---------------------------------------------------------------------------------------------------------------------
FAULTS = ('drop_last_row', 'stale_ring', 'tap_left', 'tap_right', 'tap_top', 'tap_bottom', 'bias_twice', 'no_accumulate', 'no_flip', 'reduce_tail', 'segment_off')


def _row_terms(mode, Uu, Vv, clamp=()):
    """-> per V row (b, y): G [B * Hv, taps, Ca, Cb], db [B * Hv, Cb] in the dtype of the operands"""
    B, Hv, Wv, Cb = Vv.shape
    G = torch.zeros(B * Hv, TAPS[mode], Uu.shape[3], Cb, dtype=Uu.dtype)
    for t, sub, _ in gathered(mode, Uu, Hv, Wv, clamp):
        G[:, t] = torch.einsum('bhwa,bhwc->bhac', sub, Vv).reshape(B * Hv, Uu.shape[3], Cb)
    return G, Vv.sum(2).reshape(B * Hv, Cb)


def fault_applies(pr, fault):
    c = pr['case']
    reg = case_regime(c)
    mf = reg['kernel'] in ('mfma', 'mfma_bf', 'wino')
    if fault == 'drop_last_row':
        return mf or reg['kernel'] in ('sw1', 'sw2', 'cin1')
    if fault == 'stale_ring':
        return mf and c['mode'] == 0 and 'cross_image' in reg['parts']
    if fault.startswith('tap_'):
        return c['mode'] == 0
    if fault == 'bias_twice':
        return mf and reg['nga'] > 1 and c['bias']
    if fault == 'no_accumulate':
        return bool(c['acc'])
    if fault == 'no_flip':
        return c['layout'] == 't' and c['mode'] != 1
    if fault == 'reduce_tail':
        return reg['reduce_tail']
    if fault == 'segment_off':
        return c['nseg'] > 1
    raise ValueError(fault)


def emulate(pr, fault=None):
    """float32 (exact on the integer problem): per-row products, summed per part of the mirror's partition, the parts summed, the start value added last.  The
    Winograd regime computes its tiles with the float32 transforms of the kernel.  -> G [taps, Ca, Cb], db [Cb] as read out of the destination"""
    c = pr['case']
    reg = case_regime(c)
    mode, B, Hv = c['mode'], c['B'], c['Hv']
    Uu, Vv = pr['Uu'], pr['Vv']
    if fault == 'segment_off':                                        # U of segment s read at segment s + 1
        Uu = Uu.roll(-(B // c['nseg']), 0)
    Uo, Vo = (bf16_round(Uu), bf16_round(Vv)) if reg['kernel'] == 'mfma_bf' else (Uu, Vv)
    clamp = (fault[4:],) if fault and fault.startswith('tap_') else ()
    rows, _ = _row_terms(mode, Uo, Vo, clamp)
    dbrows = Vv.sum(2).reshape(B * Hv, c['Cb'])
    if reg['kernel'] == 'wino' and not clamp:                        # whole images through the float32 transforms: the same partition of row pairs
        d, y = wino_tiles(Uo, Vo)
        per_pair = []
        for b in range(B):
            for yp in range(Hv // 2):
                per_pair.append(wino_wgrad_tiles(d[b:b + 1, yp:yp + 1], y[b:b + 1, yp:yp + 1]))
        rows = torch.stack(per_pair).repeat_interleave(2, 0) / 2     # (half a row pair per row: exact)
    keep = torch.ones(B * Hv, dtype=torch.bool)
    unit = 2 if reg['kernel'] == 'wino' else 1
    if reg['kernel'] in ('mfma', 'mfma_bf', 'wino'):
        rpw = reg['rows_per_wave'] * unit
        part_of = torch.arange(B * Hv) // rpw
        if fault == 'drop_last_row':
            for i in range(reg['nparts']):
                keep[min((i + 1) * rpw, B * Hv) - unit:min((i + 1) * rpw, B * Hv)] = False
        if fault == 'stale_ring':                                    # the row above the first row of an image inside a part: the last row of the image before
            for r in range(Hv, B * Hv, Hv):
                if r % rpw:
                    b = r // Hv
                    stale, _ = _row_terms(0, torch.cat([Uo[b - 1, -1:], Uo[b, :1]])[None], torch.cat([torch.zeros_like(Vo[b, :1]), Vo[b, :1]])[None])
                    rows[r, 0:3] += stale[1, 0:3]
    elif reg['kernel'] in ('sw1', 'sw2', 'cin1'):
        part_of = (torch.arange(B * Hv) % Hv) // reg['rows'] + (torch.arange(B * Hv) // Hv) * reg['nband']
        if fault == 'drop_last_row':
            for b in range(B):
                for band in range(reg['nband']):
                    keep[b * Hv + min((band + 1) * reg['rows'], Hv) - 1] = False
    else:
        part_of = torch.arange(B * Hv) * reg['nparts'] // (B * Hv)
    nparts = int(part_of.max()) + 1
    kf = keep.float()
    Gp = torch.zeros(nparts, *rows.shape[1:]).index_add_(0, part_of, rows * kf.view(-1, 1, 1, 1))
    bp = torch.zeros(nparts, c['Cb']).index_add_(0, part_of, dbrows * kf.view(-1, 1))
    if fault == 'reduce_tail':
        Gp, bp = Gp[:-1], bp[:-1]
    G, db = Gp.sum(0), bp.sum(0)
    if fault == 'bias_twice':
        db = db * 2
    if fault == 'no_flip':
        G = G.flip(0)
    if c['acc'] and fault != 'no_accumulate':
        G, db = G + pr['dw0'], db + pr['db0']
    return G, db


def wino_wgrad_tiles(d, y):
    """float32 Winograd weight gradient of the given tiles (d [.., 4, 4, Ca], y [.., 2, 2, Cb]) with the kernel's transforms"""
    bt, wa, wg = BT.float(), WA.float(), WG.float()
    P = torch.einsum('ik,bhwkla->bhwila', bt, d)
    P = torch.einsum('jl,bhwila->bhwija', bt, P)
    Q = torch.einsum('ik,bhwklc->bhwilc', wa, y)
    Q = torch.einsum('jl,bhwilc->bhwijc', wa, Q)
    M = torch.einsum('bhwija,bhwijc->ijac', P, Q)
    T = torch.einsum('ik,ijac->kjac', wg, M)
    return torch.einsum('jl,kjac->klac', wg, T).reshape(9, d.shape[-1], y.shape[-1])


# ---------------------------------------------------------------------------------------------------------------------
# measuring and asserting
# ---------------------------------------------------------------------------------------------------------------------
_OUT = os.path.join(os.path.dirname(cc._OUT), 'wgrad_errors.jsonl')             # next to conv_errors.jsonl


def check(where, case, key, ratio, log=None):
    """Assert one measured ratio error / bound (<= 1) and (log = True: on the device) append it to wgrad_errors.jsonl."""
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
