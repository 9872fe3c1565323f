"""Case table, launch arithmetic, inputs and references for rv_conv_fwd outside the persistent 3x3 and Winograd families of
csrc/conv.hip: the direct MFMA kernel conv_mfma_k (forced tiles 0x1NM, the default tile choice, the in-workgroup split-K 0x5NM) and
the small-channel kernels conv_narrow_out_k, conv_cin12_k and conv_small_k, plus the weight packing they read.

What conv_fwd_impl, launch_conv_rt, choose_tiles, pack_args_make, rv_packed_weight_floats, small_cpt and the three small kernels
decide on the host or per workgroup is restated here in Python (`conv_regime`, `packed_weight_floats`, `pack_mirror`), and every
case below carries the regime it is meant to reach.  tests/test_conv_cases.py asserts on the CPU that each case lands in its regime,
that the cases together reach every regime and every template instantiation, that torch's float32 CPU convolution meets the derived
bound and that emulated kernel faults miss it; tests/test_conv_regimes_gpu.py runs the kernels through the C ABI.  The persistent 3x3 band kernel
has its launch arithmetic and case table in tests/band_cases.py: `conv_regime` hands its calls over, and `reference` rounds the operands to bf16
where that regime says so.

Detection is by construction, as in tests/gemm_cases.py.  Every case runs two problems:
  * the INTEGER problem: inputs, weights, bias and start values from {+-1, +-2, +-3}; every partial sum is an integer below 2^24, so
    the float32 result is exact in any order and must equal the int64 reference with `==`;
  * the FLOAT problem: magnitudes uniform in [0.5, 1], random sign, against float64 of the same float32 inputs under
        |got - ref| <= 1.01 (K + f + 3) 2^-24 (conv(|x|, |w|) + |bias| + |out0|)        per element,
    K = taps * Cin the length of the fused multiply-add chain, f the extra adds (4: the fold of the four K slices of 0x5NM;
    log2(lanes per pixel): the xor shuffles of conv_narrow_out_k; 0 otherwise), 3 for the bias, the accumulate and the final rounding.
Inputs (and bn_z) live in wider buffers whose guard regions and skipped channels (in_ld > Cin) are NaN; destinations are prefilled
with PAD_BITS (the live region: the start value when accumulating) and everything but the live channels must come back bit-unchanged.
"""
import json
import math
import os

import torch
import torch.nn.functional as F

import parity_tol
from stream_cases import RV_BN_NREP, TOL_COLSUM

U = 2.0 ** -24                  # unit roundoff of float32
PAD_BITS = 0x7FC5EED5           # a NaN with a recognisable payload (int32 view)
NAN = float('nan')
GUARD = 8                       # floats of guard before and after every view (a multiple of 4: keeps the 16-byte alignment)
SUMS_GUARD = 16                 # doubles behind the statistics workspace
SUMS_MARK = -12345.0

GEOM = {0: (3, 3, 1, 1), 1: (1, 1, 1, 0), 2: (2, 2, 2, 0), 3: (1, 1, 1, 0)}          # (KH, KW, S, P) of the kernel template per mode
RV_CASE = [(nt, mt) for nt in (1, 2, 3, 4) for mt in (1, 2, 4)]                       # launch_conv_rt
RV_CASEK = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 4), (4, 1)]
RV_NARROW = [(16, 1), (8, 2), (8, 1)]                                                # conv_fwd_impl
RV_CIN12 = [(1, 16), (1, 8), (2, 8)]
RV_SMALL = {0: [(1, 16), (16, 1), (8, 2), (2, 8), (8, 1), (1, 8), (1, 48), (48, 1)], 1: [(1, 16), (16, 1)]}
NARROW_ROWS = CIN12_ROWS = 16   # output rows a workgroup walks down its column strip
CIN12_PD = 3                    # conv_cin12_k: input rows travel PD rows ahead of their use


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def frag_R(kdim):
    return 4 if kdim % 16 == 0 else (2 if kdim % 8 == 0 else 0)


def wino_packed(taps, kdim):
    return taps == 9 and kdim % 16 == 0


def packed_weight_floats(taps, kdim, ndim):
    """mirrors rv_packed_weight_floats"""
    R = frag_R(kdim)
    if R == 0:
        return taps * kdim * ndim
    return (taps + (16 if wino_packed(taps, kdim) else 0)) * (kdim // (4 * R)) * cdiv(ndim, 16) * 64 * R


def small_cpt(cin, cout, taps):
    return cout if cout < 4 else (cout if (cin <= 2 and taps > 1) else 4)


def choose_tiles(ntiles, ntile_n):
    """mirrors choose_tiles -> (NT, MT, best score).  Below 21 waves every candidate scores 0 and the first one -- the largest NT that
    divides ntile_n, with MT = 4 -- wins through `score > -1`."""
    best, best_score = (1, 1), -1
    for nt in (4, 3, 2, 1):
        if ntile_n % nt:
            continue
        for mt in (4, 2, 1):
            waves = cdiv(ntiles, mt) * (ntile_n // nt)
            reuse = (nt * mt * 100) // (nt + mt)
            fill = 100 if waves >= 2048 else (waves * 100) // 2048
            if reuse * fill > best_score:
                best_score, best = reuse * fill, (nt, mt)
    return best[0], best[1], best_score


def out_size(mode, H, W, up=(0, 0)):
    if mode == 2:
        return H // 2, W // 2
    if mode == 3:
        return 2 * H + up[0], 2 * W + up[1]
    return H, W


def _aligned(off_floats, nbytes):
    return (4 * off_floats) % nbytes == 0


def conv_regime(mode, B, H, W, Cin, Ho, Wo, Cout, in_ld=None, out_ld=None, algo=0, bias=True, accumulate=0, stats=None, z_ld=None,
                in_off=0, out_off=0, bias_off=0, z_off=0, coef_off=0):
    """What one rv_conv_fwd call does.  stats: None | 'sums' (bn_sums) | 'z' (bn_sums + bn_z + bn_coef) | 'z_only' (bn_z without bn_sums).
    The *_off are the float offsets of the pointers from a 16-byte boundary.  -> {'refused': reason} or the regime."""
    in_ld = Cin if in_ld is None else in_ld
    out_ld = Cout if out_ld is None else out_ld
    z_ld = Cout if z_ld is None else z_ld
    if stats == 'z_only':
        return {'refused': 'bn_z without bn_sums'}
    if not 0 <= mode <= 3:
        return {'refused': 'mode'}
    if mode in (0, 1) and (Ho, Wo) != (H, W) or mode == 2 and (Ho, Wo) != (H // 2, W // 2) \
            or mode == 3 and not (2 * H <= Ho <= 2 * H + 1 and 2 * W <= Wo <= 2 * W + 1):
        return {'refused': 'size'}
    R = frag_R(Cin)
    small = R == 0 or (Cout <= 2 and mode != 3)
    reg = {'refused': None, 'R': R, 'small': small, 'fallback': None, 'vec_out': out_ld % 4 == 0 and _aligned(out_off, 16)}
    KH, KW, S, P = GEOM[mode]
    if small:
        taps = 9 if mode == 0 else 1
        cpt = small_cpt(Cin, Cout, taps)
        tpp = Cout // cpt
        npix = B * Ho * Wo
        fused = Cout >= 4 and stats == 'sums'
        strips = None
        if mode == 0 and (Cin, Cout) in RV_NARROW:
            if in_ld % 4 == 0 and _aligned(in_off, 16):
                lpp = Cin // 4
                strips = ('narrow', 256 // lpp, NARROW_ROWS, 1)
                reg.update(lanes_per_pixel=lpp, store='scalar', stats_kind=None, stats='bn_stats' if stats else None)
            else:
                reg['fallback'] = 'in_ld' if in_ld % 4 else 'in'
        cin12 = mode == 0 and ((Cin == 1 and Cout in (16, 8)) or (Cin == 2 and Cout == 8 and in_ld % 2 == 0 and _aligned(in_off, 8)))
        if mode == 0 and (Cin, Cout) in RV_CIN12 and not cin12:
            reg['fallback'] = 'in_ld' if in_ld % 2 else 'in'
        if cin12:
            if stats == 'z' and not (z_ld % 4 == 0 and _aligned(z_off, 16)):
                reg['fallback'] = 'bn_z'
            elif stats == 'z' and not _aligned(coef_off, 16):
                reg['fallback'] = 'bn_coef'
            elif bias and not _aligned(bias_off, 16):
                reg['fallback'] = 'bias'
            else:
                lpp = Cout // 4
                strips = ('cin12', 256 // lpp, CIN12_ROWS, CIN12_PD)
                reg.update(lanes_per_pixel=lpp, store='vec' if reg['vec_out'] else 'scalar',
                           stats_kind={None: None, 'sums': 'fwd', 'z': 'bn_z'}[stats], stats='fused' if stats else None)
        if strips:
            kernel, pxw, rows, pd = strips
            nstrip, nband = cdiv(W, pxw), cdiv(H, rows)
            reg.update(kernel=kernel, form=(Cin, Cout), PXW=pxw, nstrip=nstrip, nband=nband, grid=B * nband * nstrip,
                       last_strip_cols=W - (nstrip - 1) * pxw, last_band_rows=H - (nband - 1) * rows, h_short=H < 2 + pd,
                       z_past_band=stats == 'z' and nband > 1, K=taps * Cin, f=int(math.log2(lpp)) if kernel == 'narrow' else 0)
            return reg
        if (Cin, Cout) not in RV_SMALL.get(mode, []):
            return {'refused': 'no small kernel'}
        cap = 1024 if fused else 4096
        threads = npix * tpp
        nblk0 = cdiv(threads, 256)
        nblk = min(nblk0, cap)
        if tpp == 1 and cpt % 4 == 0:
            rest = 'vec' if out_ld % 4 == 0 else 'scalar'
            store = set()
            if out_ld == Cout and npix >= 64:
                store.add('transpose')
            if out_ld != Cout or npix % 64:
                store.add(rest)                                      # every wave, or the last one, which is not full
        else:
            store = {'vec' if cpt % 4 == 0 and out_ld % 4 == 0 else 'scalar'}
        reg.update(kernel='small_k', form=(Cin, Cout, KH, KW), CPT=cpt, TPP=tpp, WREG=tpp > 1 and taps * Cin * cpt <= 80, cap=cap, nblk_wanted=nblk0,
                   nblk=nblk, passes=cdiv(threads, nblk * 256), second_pass_wgs=cdiv(max(0, threads - nblk * 256), 256), store=store,
                   ragged_wave=npix % 64 != 0, fold=(('shuffle' if tpp == 1 else 'lds') if fused else None),
                   stats='fused' if fused else ({'sums': 'bn_stats', 'z': 'bn_bwd_stats', None: None}[stats]), K=taps * Cin, f=0)
        return reg
    if not (in_ld % R == 0 and _aligned(in_off, 4 * R)):
        return {'refused': 'in alignment'}
    if mode == 3:
        if Cout % 16:
            return {'refused': 'scatter Cout'}
        ntile_n, Ph, Pw = 4 * Cout // 16, H + (Ho - 2 * H), W + (Wo - 2 * W)
    else:
        ntile_n, Ph, Pw = cdiv(Cout, 16), Ho, Wo
    nchunk, npix = Cin // (4 * R), B * Ph * Pw
    ntiles = cdiv(npix, 16)
    fam, f_nt, f_mt = (algo >> 8) & 15, (algo >> 4) & 15, algo & 15
    if mode == 0 and algo & ~(1 << 20) != 1 and fam not in (1, 5):   # the persistent 3x3 band kernel: tests/band_cases.py
        import band_cases
        return band_cases.band_regime(B, H, W, Cin, Cout, in_ld=in_ld, out_ld=out_ld, algo=algo, bias=bias, accumulate=accumulate, stats=stats, z_ld=z_ld,
                                      in_off=in_off, out_off=out_off)
    algo &= ~(1 << 20)                                               # bf16 operands: ignored outside the band kernel
    assert fam in (0, 1, 5), 'only the direct kernel is mirrored'
    NT, MT, score = choose_tiles(ntiles, ntile_n)
    nsteps = KH * KW * nchunk
    ks = fam == 5
    if ks:
        if mode == 0 or R != 4 or f_nt < 1 or ntile_n % f_nt or nchunk * (4 if mode == 2 else 1) < 4:
            return {'refused': 'split-K invalid'}
        NT, MT = f_nt, f_mt
        if (NT, MT) not in RV_CASEK:
            return {'refused': 'no instance'}
    if fam == 1:
        if f_nt < 1 or ntile_n % f_nt or f_mt not in (1, 2, 4) or f_nt > 4:
            return {'refused': 'tile invalid'}
        NT, MT = f_nt, f_mt
    if not ks and (NT, MT) not in RV_CASE:
        return {'refused': 'no instance'}
    gx = cdiv(ntiles, MT) if ks else cdiv(ntiles, 4 * MT)
    stores = set()
    for ncol in range(0, ntile_n * 16, 4):                           # one quad of four output channels per lane group and n-tile
        co0 = ncol % Cout if mode == 3 else ncol
        if co0 >= Cout:
            stores.add('skip')
        elif not reg['vec_out']:
            stores.add('scalar')
        else:
            stores.add('vec' if co0 + 3 < Cout else 'tail')
    reg.update(kernel='mfma_ks4' if ks else 'mfma', form=(mode, R, NT, MT), nchunk=nchunk, ntile_n=ntile_n, P=(Ph, Pw), npix=npix, ntiles=ntiles,
               tile=(NT, MT), forced=fam in (1, 5), degenerate=score == 0, score=score, grid=(gx, ntile_n // NT), xcd=gx >= 9,
               idle_waves=0 if ks else gx * 4 - cdiv(ntiles, MT), partial_tile=npix % 16 != 0, idle_tiles=cdiv(ntiles, MT) * MT - ntiles,
               stores=stores, pad_row=mode == 3 and Ho == 2 * H + 1, pad_col=mode == 3 and Wo == 2 * W + 1,
               stats={'sums': 'bn_stats', 'z': 'bn_bwd_stats', None: None}[stats], K=KH * KW * Cin, f=4 if ks else 0)
    if ks:
        sl = [((w * nsteps) // 4, ((w + 1) * nsteps) // 4) for w in range(4)]
        reg.update(nsteps=nsteps, slices=sl, mid_tap=any(lo % nchunk for lo, _ in sl), ragged=len({hi - lo for lo, hi in sl}) > 1,
                   deal=sorted({q % 4 for q in range(NT * MT)}))
    return reg


# ---------------------------------------------------------------------------------------------------------------------
# weight packing: logical Wm[tap][k][n] <-> the PyTorch-layout buffer <-> the packed buffer
# ---------------------------------------------------------------------------------------------------------------------
def logical_weights(w, taps, kdim, ndim, s_k, s_n, flip, scatter):
    """value(tap, k, n) of rv_pack_weights as a [taps, kdim, ndim] tensor (include/reconvat_hip.h)"""
    tap = torch.arange(taps).view(-1, 1, 1)
    k = torch.arange(kdim).view(1, -1, 1)
    n = torch.arange(ndim).view(1, 1, -1)
    if scatter:
        assert taps == 1
        idx = k * s_k + (n % scatter) * s_n + n // scatter + 0 * tap
    else:
        idx = k * s_k + n * s_n + ((taps - 1 - tap) if flip else tap)
    return w[idx]


def _frag_coords(total, R, ntile_n, nchunk):
    idx = torch.arange(total)
    r = idx % R
    t = idx // R
    lane = t % 64
    t = t // 64
    nt = t % ntile_n
    t = t // ntile_n
    c = t % nchunk
    tap = t // nchunk
    return tap, c * 4 * R + (lane // 16) * R + r, nt * 16 + lane % 16


WINO_G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)


def pack_mirror(w, taps, kdim, ndim, s_k, s_n, flip, scatter, plain):
    """mirrors pack_plain_elem / pack_frag_elem / pack_wino_elem: the packed buffer as float32"""
    Wm = logical_weights(w, taps, kdim, ndim, s_k, s_n, flip, scatter)
    R = 0 if plain else frag_R(kdim)
    if R == 0:
        assert not scatter
        return Wm.reshape(-1).clone()
    nchunk, ntile_n = kdim // (4 * R), cdiv(ndim, 16)

    def frag(W3):
        tap, k, n = _frag_coords(W3.shape[0] * nchunk * ntile_n * 64 * R, R, ntile_n, nchunk)
        ok = (k < kdim) & (n < ndim)
        return torch.where(ok, W3[tap, k.clamp(max=kdim - 1), n.clamp(max=ndim - 1)], torch.zeros(()))
    out = frag(Wm)
    if wino_packed(taps, kdim) and not scatter:
        g = Wm.double().view(3, 3, kdim, ndim)
        Uw = torch.einsum('ay,bx,yxkn->abkn', WINO_G, WINO_G, g).reshape(16, kdim, ndim).float()
        out = torch.cat([out, frag(Uw)])
    return out


def unpack_mirror(packed, taps, kdim, ndim, plain):
    """the inverse of pack_mirror's tap section: -> Wm [taps, kdim, ndim]"""
    R = 0 if plain else frag_R(kdim)
    if R == 0:
        return packed.view(taps, kdim, ndim).clone()
    nchunk, ntile_n = kdim // (4 * R), cdiv(ndim, 16)
    total = taps * nchunk * ntile_n * 64 * R
    tap, k, n = _frag_coords(total, R, ntile_n, nchunk)
    ok = (k < kdim) & (n < ndim)
    Wm = torch.full((taps, kdim, ndim), NAN)
    Wm[tap[ok], k[ok], n[ok]] = packed[:total][ok]
    return Wm


def pack_args_of(kind, which, cin, cout):
    """the rv_pack_weights arguments ops._pack_make passes -> (taps, kdim, ndim, s_k, s_n, flip, scatter, plain)"""
    scatter = 0
    if kind == 'c3':
        a = (9, cin, cout, 9, cin * 9, 0) if which == 'fwd' else (9, cout, cin, cin * 9, 9, 1)
    elif kind == 't3':
        a = (9, cin, cout, cout * 9, 9, 1) if which == 'fwd' else (9, cout, cin, 9, cout * 9, 0)
    elif kind == 'c1':
        a = (1, cin, cout, 1, cin, 0) if which == 'fwd' else (1, cout, cin, cin, 1, 0)
    elif kind == 'down':
        if which == 'fwd':
            a = (4, cin, cout, 4, cin * 4, 0)
        else:
            a, scatter = (1, cout, 4 * cin, cin * 4, 4, 0), cin
    else:
        if which == 'fwd':
            a, scatter = (1, cin, 4 * cout, cout * 4, 4, 0), cout
        else:
            a = (4, cout, cin, 4, cout * 4, 0)
    plain = 1 if (a[1] % 8 != 0 or (a[2] <= 2 and not scatter)) else 0
    return a + (scatter, plain)


# ---------------------------------------------------------------------------------------------------------------------
# references: the definition in the header comment of csrc/conv.hip
# ---------------------------------------------------------------------------------------------------------------------
def conv_ref(mode, x, Wm, bias, Ho, Wo, Cout, clamp=False):
    """x [B, H, W, Cin], Wm [taps, Cin, N] (scatter: N = 4 Cout, n = tap4 * Cout + co), bias [Cout] or None -> [B, Ho, Wo, Cout] in the
    dtype of x (float64, float32 or int64).  gather: a loop over the taps with zeros outside the image (clamp: the emulated fault, the
    value at the clamped address instead); scatter: the rows / columns past 2H / 2W receive the bias only."""
    KH, KW, S, P = GEOM[mode]
    B, H, W, Cin = x.shape
    out = torch.zeros(B, Ho, Wo, Cout, dtype=x.dtype)
    if mode == 3:
        y = (x.reshape(-1, Cin) @ Wm[0]).view(B, H, W, 4, Cout)
        for t in range(4):
            out[:, (t >> 1):2 * H:2, (t & 1):2 * W:2] = y[:, :, :, t]
    else:
        oy, ox = torch.arange(Ho), torch.arange(Wo)
        for ky in range(KH):
            for kx in range(KW):
                iy, ix = oy * S - P + ky, ox * S - P + kx
                ok = ((iy >= 0) & (iy < H)).view(-1, 1) & ((ix >= 0) & (ix < W)).view(1, -1)
                sub = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
                if not clamp:
                    sub = sub * ok.view(1, Ho, Wo, 1).to(x.dtype)
                out += sub @ Wm[ky * KW + kx]
    if bias is not None:
        out += bias
    return out


def torch_conv(mode, x, Wm, bias, Ho, Wo, Cout):
    """the same through torch.nn.functional (in the dtype of x)"""
    KH, KW, S, P = GEOM[mode]
    B, H, W, Cin = x.shape
    xn = x.permute(0, 3, 1, 2)
    if mode == 3:
        w = Wm[0].view(Cin, 4, Cout).permute(0, 2, 1).reshape(Cin, Cout, 2, 2)
        y = F.conv_transpose2d(xn, w, bias, stride=2, output_padding=(Ho - 2 * H, Wo - 2 * W))
    else:
        w = Wm.view(KH, KW, Cin, Cout).permute(3, 2, 0, 1)
        y = F.conv2d(xn, w, bias, stride=S, padding=P)
    return y.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}


def _case(name, mode, grid, cin, cout, algo=0, up=(0, 0), bias=True, acc=0, in_pad=0, out_pad=0, bias_off=0, stats=None, z_pad=0, slope=0.01,
          refusal=None, regime=None, in_off=0, z_off=0, coef_off=0):
    """grid: (B, H, W) of the INPUT.  in_pad / out_pad / z_pad: floats of padding per pixel; bias_off: float offset of the bias pointer from a 16-byte
    boundary (in_off, z_off, coef_off: the same for in, bn_z, bn_coef); stats: None | 'sums' | 'z'.  refusal: the call must return non-zero for this reason."""
    assert name not in CASES, name
    B, H, W = grid
    Ho, Wo = out_size(mode, H, W, up)
    CASES[name] = {'name': name, 'seed': len(CASES) + 1, 'mode': mode, 'B': B, 'H': H, 'W': W, 'Ho': Ho, 'Wo': Wo, 'cin': cin, 'cout': cout, 'algo': algo,
                   'bias': bias, 'acc': acc, 'in_pad': in_pad, 'out_pad': out_pad, 'bias_off': bias_off, 'stats': stats, 'z_pad': z_pad, 'slope': slope,
                   'in_off': in_off, 'z_off': z_off, 'coef_off': coef_off, 'refusal': refusal, 'regime': regime or {}}


def case_regime(case, algo=None):
    c = case
    return conv_regime(c['mode'], c['B'], c['H'], c['W'], c['cin'], c['Ho'], c['Wo'], c['cout'], in_ld=c['cin'] + c['in_pad'], out_ld=c['cout'] + c['out_pad'],
                       algo=c['algo'] if algo is None else algo, bias=c['bias'], accumulate=c['acc'], stats=c['stats'], z_ld=c['cout'] + c['z_pad'],
                       bias_off=c['bias_off'], in_off=c['in_off'], z_off=c['z_off'], coef_off=c['coef_off'], out_off=c.get('out_off', 0))


# 1. the direct MFMA kernel with forced tiles 0x1NM -------------------------------------------------------------------------------
# pixel grids per mode: T one pixel, S 70 px (a partial last tile; at MT = 1 a second workgroup of which three waves return), L 558 px
# (at MT = 1 nine workgroups: xcd_remap is not the identity).  Mode 2 reads odd inputs (the last row and column are never read).
IN_GRID = {0: {'T': (1, 1, 1), 'S': (2, 5, 7), 'L': (2, 9, 31)}, 1: {'T': (1, 1, 1), 'S': (2, 5, 7), 'L': (2, 9, 31)},
           2: {'T': (1, 3, 3), 'S': (2, 11, 15), 'L': (2, 19, 63)}, 3: {'T': (1, 1, 1), 'S': (2, 5, 7), 'L': (2, 9, 31)}}
NPIX = {'T': 1, 'S': 70, 'L': 558}                                  # (mode 3 with a padding row / column: see UPS)
NTILES = {'T': 1, 'S': 5, 'L': 35}
GRID_X = {('T', 1): 1, ('T', 2): 1, ('T', 4): 1, ('S', 1): 2, ('S', 2): 1, ('S', 4): 1, ('L', 1): 9, ('L', 2): 5, ('L', 4): 3}
IDLE_WAVES = {('T', 1): 3, ('T', 2): 3, ('T', 4): 3, ('S', 1): 3, ('S', 2): 1, ('S', 4): 2, ('L', 1): 1, ('L', 2): 2, ('L', 4): 3}
UPS = {(0, 0): 70, (0, 1): 80, (1, 0): 84, (1, 1): 96}              # mode 3, 5x7 -> 10x14, 10x15, 11x14, 11x15: B * Ph * Pw
# (Cin, Cout): R = 2 for Cin in {8, 24}, R = 4 for {16, 32}; Cout 6 and 18 are legal by the ABI though no model layer has them (the scalar tail)
PAIRS = {m: [(8, 16), (24, 24), (16, 32), (32, 48), (16, 64), (8, 6), (16, 18)] for m in (0, 1, 2)}
PAIRS[3] = [(8, 16), (24, 32), (16, 48), (32, 16)]
NTILE_N = {16: 1, 24: 2, 32: 2, 48: 3, 64: 4, 6: 1, 18: 2}           # gather; the scatter form has 4 Cout / 16
STORES = {16: {'vec'}, 32: {'vec'}, 48: {'vec'}, 64: {'vec'}, 24: {'vec', 'skip'}, 6: {'vec', 'tail', 'skip'}, 18: {'vec', 'tail', 'skip'}}
DIRECT_ALGO = {0: 1, 1: 0, 2: 0, 3: 0}                               # algo 0 of mode 0 is the persistent 3x3 kernel: the direct default is algo 1


def _tiles_for(mode, cout):
    n = 4 * cout // 16 if mode == 3 else NTILE_N[cout]
    return [(nt, mt) for nt, mt in RV_CASE if n % nt == 0]


def _forced(nt, mt):
    return 0x100 | nt << 4 | mt


_rr = 0
for _m in range(4):
    for _ci, _co in PAIRS[_m]:
        for _v, _kw in (('plain', {}), ('acc', {'acc': 1}), ('nobias', {'bias': False})):
            _t = _tiles_for(_m, _co)
            _nt, _mt = _t[_rr % len(_t)]
            _rr += 1
            _up = list(UPS)[_rr % 4] if _m == 3 else (0, 0)
            # Cout = 6, 18: a dense destination has out_ld % 4 != 0 and stores scalars; the tail `co0 + 3 >= Cout` of the 16-byte path needs out_ld = Cout + 2
            _pad = 2 if _co in (6, 18) and _v != 'nobias' else 0
            _st = {'vec'} if _m == 3 else (STORES[_co] if _pad or _co % 4 == 0 else {'scalar', 'skip'})
            _case('direct m%d %d->%d S %s' % (_m, _ci, _co, _v), _m, IN_GRID[_m]['S'], _ci, _co, _forced(_nt, _mt), up=_up, out_pad=_pad,
                  regime={'kernel': 'mfma', 'R': 2 if _ci in (8, 24) else 4, 'tile': (_nt, _mt), 'npix': UPS[_up], 'partial_tile': UPS[_up] % 16 != 0,
                          'stores': _st, 'pad_row': _up[0] == 1, 'pad_col': _up[1] == 1, 'forced': True}, **_kw)
    # every (NT, MT) of RV_CASE on the one-pixel and on the 558-pixel grid
    for _i, (_nt, _mt) in enumerate(RV_CASE):
        _g = 'TL'[_i % 2] if _mt != 1 else 'L'                        # MT = 1 on the large grid: nine workgroups
        _ok = [p for p in PAIRS[_m] if (4 * p[1] // 16 if _m == 3 else NTILE_N[p[1]]) % _nt == 0]
        _ci, _co = _ok[(_i + _m) % len(_ok)]
        _case('direct m%d %d->%d %s nt%d mt%d' % (_m, _ci, _co, _g, _nt, _mt), _m, IN_GRID[_m][_g], _ci, _co, _forced(_nt, _mt), acc=_i % 2,
              regime={'kernel': 'mfma', 'tile': (_nt, _mt), 'npix': NPIX[_g], 'ntiles': NTILES[_g], 'xcd': GRID_X[(_g, _mt)] >= 9,
                      'idle_waves': IDLE_WAVES[(_g, _mt)], 'partial_tile': True})
    for _g in 'TSL':                                                 # all three grids at (1, 1) and MT in {2, 4}: the early return of whole waves
        for _mt in (1, 2, 4):
            _ci, _co = PAIRS[_m][(_mt + _m) % 4]
            _case('direct m%d %d->%d %s waves mt%d' % (_m, _ci, _co, _g, _mt), _m, IN_GRID[_m][_g], _ci, _co, _forced(1, _mt),
                  regime={'kernel': 'mfma', 'tile': (1, _mt), 'grid': (GRID_X[(_g, _mt)], 4 * _co // 16 if _m == 3 else NTILE_N[_co]),
                          'idle_waves': IDLE_WAVES[(_g, _mt)]})
    # pixel strides: in_ld = Cin + 4R, out_ld = Cout + 4 (16-byte stores into a channel slice), out_ld = Cout + 1 (the scalar path)
    _ci, _co = PAIRS[_m][2 * (_m % 2)]                               # (8, 16) or (16, 32 / 48): every quad of Cout is stored
    _R = 2 if _ci in (8, 24) else 4
    _case('direct m%d %d->%d S in_ld' % (_m, _ci, _co), _m, IN_GRID[_m]['S'], _ci, _co, _forced(1, 2), in_pad=4 * _R, regime={'kernel': 'mfma', 'stores': {'vec'}, 'R': _R})
    _case('direct m%d %d->%d S out_ld+4' % (_m, _ci, _co), _m, IN_GRID[_m]['S'], _ci, _co, _forced(1, 1), out_pad=4, acc=1, regime={'kernel': 'mfma', 'stores': {'vec'}})
    _case('direct m%d %d->%d S out_ld+1' % (_m, _ci, _co), _m, IN_GRID[_m]['S'], _ci, _co, _forced(1, 4), out_pad=1, acc=1, regime={'kernel': 'mfma', 'stores': {'scalar'}})
    if _m != 3:
        _case('direct m%d 16->18 S out_ld+1' % _m, _m, IN_GRID[_m]['S'], 16, 18, _forced(2, 2), out_pad=1, regime={'kernel': 'mfma', 'stores': {'scalar', 'skip'}})

_case('direct m1 16->32 8x8 whole tiles', 1, (1, 8, 8), 16, 32, _forced(2, 1), regime={'kernel': 'mfma', 'npix': 64, 'partial_tile': False, 'idle_waves': 0, 'idle_tiles': 0})

# 2. the default tile choice: below 21 waves every score is 0 and (max NT dividing ntile_n, 4) wins; one case where the score decides
for _m in range(4):
    _co = 16 if _m == 3 else 48                                      # 5 tiles x 4 (x 3) n-tiles: 20 (15) waves at (1, 1)
    _case('default m%d 16->%d S' % (_m, _co), _m, IN_GRID[_m]['S'], 16, _co, DIRECT_ALGO[_m], regime={'kernel': 'mfma', 'tile': (4 if _m == 3 else 3, 4), 'degenerate': True, 'forced': False})
    _co = 48 if _m == 3 else 32
    _case('default m%d 8->%d T' % (_m, _co), _m, IN_GRID[_m]['T'], 8, _co, DIRECT_ALGO[_m], acc=1, regime={'kernel': 'mfma', 'tile': (4 if _m == 3 else 2, 4), 'degenerate': True, 'forced': False})
_case('default m1 16->192 scored', 1, (3, 33, 42), 16, 192, 0, regime={'kernel': 'mfma', 'tile': (2, 1), 'degenerate': False, 'forced': False, 'ntiles': 260, 'xcd': True})

# 3. the in-workgroup split-K 0x5NM: Cin = 64 in mode 1 (4 steps, one per wave), Cin = 80 (5 steps: ragged slices), Cin = 32 in mode 2 (8 steps,
# two per wave: a slice boundary at a tap change, and with Cin = 48 -- 12 steps of 3 chunks -- slices that start in the middle of a tap)
_KS = {(1, 64): [(0, 1), (1, 2), (2, 3), (3, 4)], (1, 80): [(0, 1), (1, 2), (2, 3), (3, 5)], (3, 64): [(0, 1), (1, 2), (2, 3), (3, 4)],
       (3, 80): [(0, 1), (1, 2), (2, 3), (3, 5)], (2, 32): [(0, 2), (2, 4), (4, 6), (6, 8)], (2, 48): [(0, 3), (3, 6), (6, 9), (9, 12)],
       (2, 80): [(0, 5), (5, 10), (10, 15), (15, 20)]}
_DEAL = {(1, 1): [0], (1, 2): [0, 1], (2, 1): [0, 1], (2, 2): [0, 1, 2, 3], (1, 4): [0, 1, 2, 3], (4, 1): [0, 1, 2, 3]}
for _m, _cins in ((1, (64, 80)), (2, (32, 48, 80)), (3, (64, 80))):
    for _i, (_nt, _mt) in enumerate(RV_CASEK):
        _ci = _cins[_i % len(_cins)]
        _co = 16 if _m == 3 else 64
        _g = 'SL'[_i % 2]
        _kw = {'acc': 1} if _i == 1 else ({'out_pad': 4} if _i == 2 else ({'bias': False} if _i == 3 else {}))
        _case('splitk m%d %d->%d %s nt%d mt%d' % (_m, _ci, _co, _g, _nt, _mt), _m, IN_GRID[_m][_g], _ci, _co, 0x500 | _nt << 4 | _mt, **_kw,
              regime={'kernel': 'mfma_ks4', 'tile': (_nt, _mt), 'slices': _KS[(_m, _ci)], 'deal': _DEAL[(_nt, _mt)], 'npix': NPIX[_g], 'f': 4,
                      'mid_tap': _m != 2})       # the one tap of modes 1 and 3: waves 1 .. 3 start at a chunk > 0; mode 2: every slice is one whole tap
_case('splitk m2 16->64 S one step per wave', 2, IN_GRID[2]['S'], 16, 64, 0x511, regime={'kernel': 'mfma_ks4', 'nsteps': 4, 'mid_tap': False})
# the refusals: mode 0, R = 2, fewer than 4 steps, an NT that does not divide ntile_n
_case('splitk refused mode 0', 0, IN_GRID[0]['S'], 64, 64, 0x511, refusal='split-K invalid')
_case('splitk refused R2', 1, IN_GRID[1]['S'], 72, 64, 0x511, refusal='split-K invalid')
_case('splitk refused 3 steps', 1, IN_GRID[1]['S'], 48, 64, 0x511, refusal='split-K invalid')
_case('splitk refused NT', 1, IN_GRID[1]['S'], 64, 48, 0x521, refusal='split-K invalid')

# 4. conv_narrow_out_k: a last strip of one column, a last band of one row; one pixel; 2 x 3 pixels
_NARROW_BIG = {(16, 1): (2, 17, 65), (8, 2): (2, 17, 129), (8, 1): (2, 17, 129)}
for (_ci, _co), _big in _NARROW_BIG.items():
    _lab = {'kernel': 'narrow', 'form': (_ci, _co), 'PXW': 1024 // _ci, 'nstrip': 2, 'nband': 2, 'last_strip_cols': 1, 'last_band_rows': 1, 'store': 'scalar',
            'f': 2 if _ci == 16 else 1}
    _case('narrow %d->%d big' % (_ci, _co), 0, _big, _ci, _co, regime=_lab)
    _case('narrow %d->%d big nobias out_ld+3' % (_ci, _co), 0, _big, _ci, _co, bias=False, out_pad=3, regime=_lab)
    _case('narrow %d->%d big acc out_ld+3 in_ld+4' % (_ci, _co), 0, _big, _ci, _co, acc=1, out_pad=3, in_pad=4, regime=_lab)
    for _g in ((1, 1, 1), (1, 2, 3)):
        _lab = {'kernel': 'narrow', 'form': (_ci, _co), 'nstrip': 1, 'nband': 1, 'last_strip_cols': _g[2], 'last_band_rows': _g[1], 'h_short': True}
        _case('narrow %d->%d %dx%d' % (_ci, _co, _g[1], _g[2]), 0, _g, _ci, _co, regime=_lab)
        _case('narrow %d->%d %dx%d acc nobias out_ld+3' % (_ci, _co, _g[1], _g[2]), 0, _g, _ci, _co, acc=1, bias=False, out_pad=3, regime=_lab)

# 5. conv_cin12_k: the same strips and bands; H below the 2 + PD rows in flight; both statistics kinds; z one row past the band
_CIN12_BIG = {(1, 16): (2, 17, 65), (1, 8): (2, 17, 129), (2, 8): (2, 17, 129)}
for (_ci, _co), _big in _CIN12_BIG.items():
    _lab = {'kernel': 'cin12', 'form': (_ci, _co), 'PXW': 1024 // _co, 'nstrip': 2, 'nband': 2, 'last_strip_cols': 1, 'last_band_rows': 1, 'h_short': False}
    _case('cin12 %d->%d big' % (_ci, _co), 0, _big, _ci, _co, regime=dict(_lab, store='vec', stats_kind=None))
    _case('cin12 %d->%d big sums' % (_ci, _co), 0, _big, _ci, _co, stats='sums', regime=dict(_lab, store='vec', stats_kind='fwd', stats='fused'))
    _case('cin12 %d->%d big z' % (_ci, _co), 0, _big, _ci, _co, stats='z', bias=False, regime=dict(_lab, stats_kind='bn_z', stats='fused', z_past_band=True))
    _case('cin12 %d->%d big z_ld+4' % (_ci, _co), 0, _big, _ci, _co, stats='z', z_pad=4, in_pad=2, regime=dict(_lab, stats_kind='bn_z', z_past_band=True))
    _case('cin12 %d->%d big acc' % (_ci, _co), 0, _big, _ci, _co, acc=1, out_pad=4, regime=dict(_lab, store='vec'))
    _case('cin12 %d->%d big scalar sums' % (_ci, _co), 0, _big, _ci, _co, out_pad=1, stats='sums', acc=1, regime=dict(_lab, store='scalar', stats_kind='fwd'))
    for _h in (1, 2, 4):
        _lab = {'kernel': 'cin12', 'form': (_ci, _co), 'nstrip': 1, 'nband': 1, 'last_band_rows': _h, 'h_short': True}
        _case('cin12 %d->%d H%d sums' % (_ci, _co, _h), 0, (1, _h, 5), _ci, _co, stats='sums', regime=dict(_lab, stats_kind='fwd'))
        _case('cin12 %d->%d H%d z_ld+4' % (_ci, _co, _h), 0, (1, _h, 5), _ci, _co, stats='z', z_pad=4, regime=dict(_lab, stats_kind='bn_z', z_past_band=False))
        _case('cin12 %d->%d H%d acc scalar' % (_ci, _co, _h), 0, (1, _h, 5), _ci, _co, acc=1, out_pad=1, bias=False, regime=dict(_lab, store='scalar'))

# 6. conv_small_k.  From the kernel text: (a) the 16-byte loads of the CIN % 4 == 0 form are plain `*reinterpret_cast<const f32x4*>(src + c)`
# global loads of an address that is 4-byte aligned for any in_ld -- the unaligned 16-byte global loads rv_gemm already issues for its odd leading
# dimensions (gemm.hip: f32x4u); (b) every tap address is `centre + (cy * W + cx) * in_ld` with cy, cx clamped into [0, H) x [0, W) and at most CIN
# floats read from it, so every load lies inside the view; out-of-image taps are zeroed by a select afterwards.
_SMALL_BIG = (2, 17, 65)            # 2210 px: 34 full waves and one of 34 lanes
# the fallbacks behind conv_narrow_out_k (in_ld = Cin + 1) and conv_cin12_k (in_ld = 3 for 2 -> 8; a bias 4 bytes off a 16-byte boundary for 1 -> 16, 1 -> 8)
for _ci, _co in RV_NARROW:
    for _g in (_SMALL_BIG, (1, 1, 1)):
        _lab = {'kernel': 'small_k', 'form': (_ci, _co, 3, 3), 'fallback': 'in_ld', 'CPT': _co, 'TPP': 1, 'WREG': False, 'store': {'scalar'}, 'passes': 1}
        _case('small fallback %d->%d %dx%d in_ld+1' % (_ci, _co, _g[1], _g[2]), 0, _g, _ci, _co, in_pad=1, acc=int(_g[1] == 1), regime=_lab)
for (_ci, _co), _kw, _why in (((2, 8), {'in_pad': 1}, 'in_ld'), ((1, 16), {'bias_off': 1}, 'bias'), ((1, 8), {'bias_off': 1}, 'bias')):
    _lab = {'kernel': 'small_k', 'form': (_ci, _co, 3, 3), 'fallback': _why, 'CPT': _co, 'TPP': 1, 'WREG': False}
    _case('small fallback %d->%d big' % (_ci, _co), 0, _SMALL_BIG, _ci, _co, regime=dict(_lab, store={'transpose', 'vec'}, ragged_wave=True, fold=None), **_kw)
    _case('small fallback %d->%d big sums' % (_ci, _co), 0, _SMALL_BIG, _ci, _co, stats='sums', regime=dict(_lab, store={'transpose', 'vec'}, fold='shuffle', stats='fused'), **_kw)
    _case('small fallback %d->%d big out_ld+4 acc' % (_ci, _co), 0, _SMALL_BIG, _ci, _co, out_pad=4, acc=1, regime=dict(_lab, store={'vec'}), **_kw)
    _case('small fallback %d->%d big out_ld+1 sums' % (_ci, _co), 0, _SMALL_BIG, _ci, _co, out_pad=1, stats='sums', regime=dict(_lab, store={'scalar'}, fold='shuffle'), **_kw)
    _case('small fallback %d->%d 1x1 sums' % (_ci, _co), 0, (1, 1, 1), _ci, _co, stats='sums', regime=dict(_lab, store={'vec'}, fold='shuffle'), **_kw)
    _case('small fallback %d->%d 64 px' % (_ci, _co), 0, (1, 4, 16), _ci, _co, regime=dict(_lab, store={'transpose'}, ragged_wave=False), **_kw)
# ... and through the alignment of `in` (16 bytes for the narrow kernels, 8 for 2 -> 8), of bn_z and of bn_coef
_case('small fallback 16->1 2x3 in+4B', 0, (1, 2, 3), 16, 1, in_off=1, regime={'kernel': 'small_k', 'form': (16, 1, 3, 3), 'fallback': 'in'})
_case('small fallback 2->8 2x3 in+4B', 0, (1, 2, 3), 2, 8, in_off=1, regime={'kernel': 'small_k', 'form': (2, 8, 3, 3), 'fallback': 'in'})
_case('small fallback 1->8 2x3 z+4B', 0, (1, 2, 3), 1, 8, stats='z', z_off=1, regime={'kernel': 'small_k', 'fallback': 'bn_z', 'stats': 'bn_bwd_stats'})
_case('small fallback 1->16 2x3 coef+4B', 0, (1, 2, 3), 1, 16, stats='z', coef_off=1, regime={'kernel': 'small_k', 'fallback': 'bn_coef', 'stats': 'bn_bwd_stats'})
_case('small fallback 1->16 big z', 0, _SMALL_BIG, 1, 16, bias_off=1, stats='z', regime={'kernel': 'small_k', 'fallback': 'bias', 'stats': 'bn_bwd_stats', 'fold': None})
# ConvStack layer 0 and its input gradient; the 1x1 pair
for _g in (_SMALL_BIG, (1, 1, 1)):
    _t = '%dx%d' % _g[1:]
    _big = _g == _SMALL_BIG
    _lab = {'kernel': 'small_k', 'form': (1, 48, 3, 3), 'fallback': None, 'CPT': 48, 'TPP': 1, 'WREG': False}
    _case('small 1->48 %s' % _t, 0, _g, 1, 48, regime=dict(_lab, store={'transpose', 'vec'} if _big else {'vec'}, fold=None))
    _case('small 1->48 %s sums acc' % _t, 0, _g, 1, 48, stats='sums', acc=1, regime=dict(_lab, fold='shuffle', stats='fused'))
    _case('small 1->48 %s out_ld+4 nobias' % _t, 0, _g, 1, 48, out_pad=4, bias=False, regime=dict(_lab, store={'vec'}))
    _case('small 1->48 %s out_ld+1' % _t, 0, _g, 1, 48, out_pad=1, regime=dict(_lab, store={'scalar'}))
    _lab = {'kernel': 'small_k', 'form': (48, 1, 3, 3), 'fallback': None, 'CPT': 1, 'TPP': 1, 'store': {'scalar'}}
    _case('small 48->1 %s' % _t, 0, _g, 48, 1, regime=_lab)
    _case('small 48->1 %s acc nobias in_ld+1 out_ld+3' % _t, 0, _g, 48, 1, acc=1, bias=False, in_pad=1, out_pad=3, regime=_lab)
    _lab = {'kernel': 'small_k', 'form': (1, 16, 1, 1), 'fallback': None, 'CPT': 4, 'TPP': 4, 'WREG': True}
    _case('small 1x1 1->16 %s' % _t, 1, _g, 1, 16, regime=dict(_lab, store={'vec'}, fold=None))
    _case('small 1x1 1->16 %s sums' % _t, 1, _g, 1, 16, stats='sums', in_pad=1, regime=dict(_lab, store={'vec'}, fold='lds', stats='fused'))
    _case('small 1x1 1->16 %s out_ld+1 sums acc' % _t, 1, _g, 1, 16, stats='sums', out_pad=1, acc=1, bias=False, regime=dict(_lab, store={'scalar'}, fold='lds'))
    _lab = {'kernel': 'small_k', 'form': (16, 1, 1, 1), 'fallback': None, 'CPT': 1, 'TPP': 1, 'store': {'scalar'}}
    _case('small 1x1 16->1 %s' % _t, 1, _g, 16, 1, regime=_lab)
    _case('small 1x1 16->1 %s acc in_ld+1 out_ld+3' % _t, 1, _g, 16, 1, acc=1, in_pad=1, out_pad=3, regime=_lab)
# one grid-stride case per cap: 513 x 513 = 263169 px
_case('small stride 1->16 fallback sums', 0, (1, 513, 513), 1, 16, bias_off=1, stats='sums',
      regime={'kernel': 'small_k', 'fallback': 'bias', 'cap': 1024, 'nblk_wanted': 1029, 'nblk': 1024, 'passes': 2, 'second_pass_wgs': 5, 'fold': 'shuffle'})
_case('small stride 1x1 1->16', 1, (1, 513, 513), 1, 16,
      regime={'kernel': 'small_k', 'TPP': 4, 'cap': 4096, 'nblk_wanted': 4113, 'nblk': 4096, 'passes': 2, 'second_pass_wgs': 17, 'fold': None})
GRID_STRIDE_CASES = [n for n in CASES if n.startswith('small stride')]

# 7. the statistics passes behind the kernels that do not fuse them
_case('direct m1 16->32 L sums', 1, IN_GRID[1]['L'], 16, 32, _forced(2, 2), stats='sums', regime={'kernel': 'mfma', 'stats': 'bn_stats'})
_case('direct m2 8->16 L sums acc', 2, IN_GRID[2]['L'], 8, 16, _forced(1, 4), stats='sums', acc=1, regime={'kernel': 'mfma', 'stats': 'bn_stats'})
_case('direct m3 16->16 S z', 3, IN_GRID[3]['S'], 16, 16, _forced(4, 1), up=(1, 1), stats='z', z_pad=4, regime={'kernel': 'mfma', 'stats': 'bn_bwd_stats', 'pad_row': True})
_case('splitk m1 64->64 L z', 1, IN_GRID[1]['L'], 64, 64, 0x522, stats='z', bias=False, regime={'kernel': 'mfma_ks4', 'stats': 'bn_bwd_stats'})

RUN_CASES = [n for n, c in CASES.items() if not c['refusal']]
REFUSED_CASES = [n for n, c in CASES.items() if c['refusal']]

# 8. one pack table: (taps, kdim, ndim, layout, flip, scatter, plain).  layout 'kn': the buffer is [k][n][tap], 'nk': [n][k][tap]
PACK_TABLE = [
    ('R4 with a Winograd section', 9, 16, 32, 'nk', 0, 0, 0),
    ('R2', 4, 24, 16, 'nk', 0, 0, 0),
    ('plain', 9, 1, 16, 'nk', 0, 0, 0),
    ('flipped', 9, 32, 16, 'kn', 1, 0, 0),
    ('scatter', 1, 16, 64, 'kn', 0, 16, 0),
    ('ndim 18', 1, 16, 18, 'kn', 0, 0, 0),
    ('forced plain, flipped', 9, 8, 2, 'kn', 1, 0, 1),
]


def pack_entry(i, kind='int'):
    """-> (w buffer float32, rv_pack_weights arguments (taps, kdim, ndim, s_k, s_n, flip, scatter, plain))"""
    _, taps, kdim, ndim, layout, flip, scatter, plain = PACK_TABLE[i]
    n_src, t_src = (scatter, 4) if scatter else (ndim, taps)
    s_k, s_n = (n_src * t_src, t_src) if layout == 'kn' else (t_src, kdim * t_src)
    w = _draw(_gen(7000 + i, kind == 'int'), kind, kdim * n_src * t_src)
    if kind == 'int':
        w = w * 4                                                    # multiples of 4: G g G^T is exact
    return w, (taps, kdim, ndim, s_k, s_n, flip, scatter, plain)


def pack_floats(args):
    taps, kdim, ndim, _, _, _, _, plain = args
    return taps * kdim * ndim if plain else packed_weight_floats(taps, kdim, ndim)


# ---------------------------------------------------------------------------------------------------------------------
# inputs (CPU, seeded per case, cached, never modified by the tests)
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


def _nan_buffer(n):
    return torch.full((n,), NAN)


def _pad_buffer(n):
    buf = torch.empty(n, dtype=torch.float32)
    buf.view(torch.int32).fill_(PAD_BITS)
    return buf


def nhwc_view(buf, off, B, H, W, C, ld):
    return torch.as_strided(buf, (B, H, W, C), (H * W * ld, W * ld, ld, 1), off)


def case_pack_args(case):
    """the weight buffer layout of a case: [k][n][tap] or [n][k][tap] by the seed, flipped taps on every third 3x3 / 2x2 case"""
    mode, cin, cout = case['mode'], case['cin'], case['cout']
    taps = GEOM[mode][0] * GEOM[mode][1]
    small = frag_R(cin) == 0 or (cout <= 2 and mode != 3)
    scatter = cout if mode == 3 else 0
    ndim, n_src, t_src = (4 * cout, cout, 4) if mode == 3 else (cout, cout, taps)
    s_k, s_n = (n_src * t_src, t_src) if case['seed'] % 2 else (t_src, cin * t_src)
    return taps, cin, ndim, s_k, s_n, 1 if (taps > 1 and case['seed'] % 3 == 0) else 0, scatter, 1 if small else 0


_problems = {}


def problem(case, kind):
    """One problem of a case: the logical tensors x [B, H, W, Cin], Wm [taps, Cin, N], bias [Cout], out0 [B, Ho, Wo, Cout], z and coef, and the flat host
    buffers they live in, with the float offsets (`*_at`) of the views."""
    key = (case['name'], kind)
    if key in _problems:
        return _problems[key]
    c = case
    B, H, W, Ho, Wo, cin, cout = c['B'], c['H'], c['W'], c['Ho'], c['Wo'], c['cin'], c['cout']
    g = _gen(c['seed'], kind == 'int')
    args = case_pack_args(c)
    taps, kdim, ndim, s_k, s_n, flip, scatter, plain = args
    n_src, t_src = (cout, 4) if scatter else (ndim, taps)
    pr = {'case': c, 'kind': kind, 'pack_args': args, 'in_ld': cin + c['in_pad'], 'out_ld': cout + c['out_pad'], 'z_ld': cout + c['z_pad']}
    pr['w_buf'] = _draw(g, kind, kdim * n_src * t_src)
    pr['Wm'] = logical_weights(pr['w_buf'], *args[:7])
    pr['x'] = _draw(g, kind, B, H, W, cin)
    pr['bias'] = _draw(g, kind, cout) if c['bias'] else None
    pr['out0'] = _draw(g, kind, B, Ho, Wo, cout) if c['acc'] else None
    pr['in_at'] = GUARD + c['in_off']
    pr['in_buf'] = _nan_buffer(pr['in_at'] + B * H * W * pr['in_ld'] + GUARD)
    nhwc_view(pr['in_buf'], pr['in_at'], B, H, W, cin, pr['in_ld']).copy_(pr['x'])
    if c['bias']:
        pr['bias_at'] = GUARD + c['bias_off']
        pr['bias_buf'] = _nan_buffer(GUARD + c['bias_off'] + cout + GUARD)
        pr['bias_buf'][pr['bias_at']:pr['bias_at'] + cout] = pr['bias']
    pr['out_at'] = GUARD + c.get('out_off', 0)                       # (out_off: the band cases of tests/band_cases.py)
    pr['out_buf'] = _pad_buffer(pr['out_at'] + B * Ho * Wo * pr['out_ld'] + GUARD)
    if c['acc']:
        nhwc_view(pr['out_buf'], pr['out_at'], B, Ho, Wo, cout, pr['out_ld']).copy_(pr['out0'])
    if c['stats'] == 'z':
        # z, and coef = [mean | invstd | scale | shift | var]: |z * scale| >= 0.25 and |shift| <= 0.1, so z * scale + shift stays 0.15 away from the kink
        gz = _gen(c['seed'], 77)
        pr['z'] = _draw(gz, 'float', B, Ho, Wo, cout)
        coef = torch.stack([0.2 * _draw(gz, 'float', cout), 0.5 + _draw(gz, 'float', cout).abs(), _draw(gz, 'float', cout), 0.1 * _draw(gz, 'float', cout),
                            _draw(gz, 'float', cout).abs()])
        pr['coef'] = coef
        pr['z_at'] = GUARD + c['z_off']
        pr['z_buf'] = _nan_buffer(pr['z_at'] + B * Ho * Wo * pr['z_ld'] + GUARD)
        nhwc_view(pr['z_buf'], pr['z_at'], B, Ho, Wo, cout, pr['z_ld']).copy_(pr['z'])
        pr['coef_at'] = GUARD + c['coef_off']
        pr['coef_buf'] = _nan_buffer(pr['coef_at'] + 5 * cout + GUARD)
        pr['coef_buf'][pr['coef_at']:pr['coef_at'] + 5 * cout] = coef.reshape(-1)
        assert (pr['z'] * coef[2] + coef[3]).abs().min().item() >= 1e-3
    if c['stats']:
        pr['sums_buf'] = torch.zeros(RV_BN_NREP * 2 * cout + SUMS_GUARD, dtype=torch.float64)
        pr['sums_buf'][RV_BN_NREP * 2 * cout:] = SUMS_MARK
    _problems[key] = pr
    return pr


def live(pr, buf):
    """the [B, Ho, Wo, Cout] view of the destination inside `buf`"""
    c = pr['case']
    return nhwc_view(buf, pr['out_at'], c['B'], c['Ho'], c['Wo'], c['cout'], pr['out_ld'])


def padding_intact(pr, buf):
    """every float of the destination buffer outside the live channels still holds PAD_BITS"""
    b = buf.detach().cpu().clone().view(torch.int32)
    live(pr, b).fill_(PAD_BITS)
    return bool((b == PAD_BITS).all().item())


# ---------------------------------------------------------------------------------------------------------------------
# references and comparisons
# ---------------------------------------------------------------------------------------------------------------------
_refs = {}


def bf16_round(t):
    """float32 -> the nearest bf16 number (ties to even) as float32: v_cvt_pk_bf16_f32"""
    return t.to(torch.bfloat16).to(torch.float32)


def reference(pr):
    """-> {'out': float64 [B, Ho, Wo, Cout] (the integer problem: computed in int64), 'bound': per element, 'mag'}"""
    key = (pr['case']['name'], pr['kind'])
    if key in _refs:
        return _refs[key]
    c = pr['case']
    reg = case_regime(c)
    dt = torch.int64 if pr['kind'] == 'int' else torch.float64
    bias = None if pr['bias'] is None else pr['bias'].to(dt)
    # bf16 operands (the band kernel under bit 20): the reference rounds x and w first, and 2K stands for K (a full ulp for each internal add of the matrix pipe)
    bf = bool(reg.get('bf'))
    x, Wm = (bf16_round(pr['x']), bf16_round(pr['Wm'])) if bf else (pr['x'], pr['Wm'])
    out = conv_ref(c['mode'], x.to(dt), Wm.to(dt), bias, c['Ho'], c['Wo'], c['cout']).double()
    mag = conv_ref(c['mode'], x.double().abs(), Wm.double().abs(), None if bias is None else pr['bias'].double().abs(), c['Ho'], c['Wo'], c['cout'])
    if c['acc']:
        out = out + pr['out0'].double()
        mag = mag + pr['out0'].double().abs()
    ref = {'out': out, 'mag': mag, 'bound': 1.01 * ((2 if bf else 1) * reg['K'] + reg['f'] + 3) * U * mag}
    _refs[key] = ref
    return ref


def err_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound in float64: 0 where they are equal (a bound of 0 asks for `==`), inf for a NaN"""
    r = ratio_map(got, ref, bound)
    return r.max().item() if r.numel() else 0.0


def ratio_map(got, ref, bound):
    got, ref = got.detach().double().cpu(), ref.double()
    d = (got - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return torch.where(torch.isnan(d), torch.full_like(d, float('inf')), r)


def compare(pr, out):
    """ratio of `out` [B, Ho, Wo, Cout] against reference(pr); <= 1 passes.  The integer problem is exact: its bound is 0."""
    ref = reference(pr)
    return err_ratio(out, ref['out'], torch.zeros_like(ref['bound']) if pr['kind'] == 'int' else ref['bound'])


def stats_reference(pr, out):
    """float64 sums of the device's own `out` as read back -> (sums [2, C], sum |term| [2, C]).  forward kind: (sum y, sum y^2); bn_z kind: (sum dd,
    sum dd * xhat) with dd = out * lrelu'(z * scale + shift), xhat = (z - mean) * invstd"""
    t1, t2 = stats_terms(pr, out)
    return torch.stack([t1.sum(0), t2.sum(0)]), torch.stack([t1.abs().sum(0), t2.abs().sum(0)])


def stats_terms(pr, out):
    """the two float64 terms [pixels, C] a pixel adds to the statistics of its channels"""
    c = pr['case']
    y = out.detach().double().cpu().reshape(-1, c['cout'])
    if c['stats'] == 'z':
        z, coef = pr['z'].double().reshape(-1, c['cout']), pr['coef'].double()
        dd = torch.where(z * coef[2] + coef[3] > 0, y, y * float(torch.tensor(c['slope'], dtype=torch.float32)))
        return dd, dd * (z - coef[0]) * coef[1]
    return y, y * y


def stats_ratio(pr, out, sums_buf, exact=None):
    """the replicas of the workspace added up against stats_reference, relative to TOL_COLSUM * sum |term| per channel; the guard behind the workspace
    must be unchanged.  exact (the integer problem, forward kind, every partial below 2^24): `==`."""
    C = pr['case']['cout']
    ws = sums_buf.detach().cpu().double()
    if not bool((ws[RV_BN_NREP * 2 * C:] == SUMS_MARK).all().item()):
        return float('inf')
    got = ws[:RV_BN_NREP * 2 * C].view(RV_BN_NREP, 2, C).sum(0)
    want, terms = stats_reference(pr, out)
    if exact is None:
        exact = pr['kind'] == 'int' and pr['case']['stats'] == 'sums' and terms.max().item() < 2 ** 24
    return err_ratio(got, want, torch.zeros_like(terms) if exact else TOL_COLSUM * terms)


# ---------------------------------------------------------------------------------------------------------------------
# float32 on the CPU, with emulated kernel faults
# ---------------------------------------------------------------------------------------------------------------------
def fault_region(pr, fault):
    """the [B, Ho, Wo, Cout] bool mask of the elements a fault moves (None: the fault does not apply to the case)"""
    c = pr['case']
    reg = case_regime(c)
    B, Ho, Wo, C = c['B'], c['Ho'], c['Wo'], c['cout']
    m = torch.zeros(B, Ho, Wo, C, dtype=torch.bool)
    if fault == 'clamp_tap':
        if c['mode'] != 0 or Ho * Wo == 1:
            return None
        m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True
    elif fault in ('last_strip', 'last_band'):
        if reg['kernel'] not in ('narrow', 'cin12'):
            return None
        if fault == 'last_strip':
            m[:, :, Wo - reg['last_strip_cols']:] = True
        else:
            m[:, Ho - reg['last_band_rows']:] = True
    elif fault == 'pad_row':
        if not reg.get('pad_row'):
            return None
        m[:, Ho - 1] = True
    elif fault == 'no_accumulate':
        if not c['acc']:
            return None
        m[:] = True
    elif fault == 'drop_slice':
        if reg['kernel'] != 'mfma_ks4':
            return None
        m[:] = True
        if reg['pad_row']:
            m[:, Ho - 1] = False
        if reg['pad_col']:
            m[:, :, Wo - 1] = False
    elif fault == 'quad_shift':
        if not (reg['kernel'] == 'small_k' and reg['TPP'] > 1 and reg['passes'] > 1):
            return None
        m.view(-1, C)[reg['nblk'] * 256 // reg['TPP']:] = True
    else:
        raise ValueError(fault)
    return m


def emulate(pr, fault=None):
    """float32: the taps added one by one with torch's float32 CPU product.  fault: None or one of fault_region's.  -> out [B, Ho, Wo, Cout] float32"""
    c = pr['case']
    reg = case_regime(c)
    Wm = pr['Wm']
    if fault == 'drop_slice':                                        # the K slice of wave 1: its steps s = tap * nchunk + chunk
        Wm = Wm.clone()
        for s in range(*reg['slices'][1]):
            Wm[s // reg['nchunk'], (s % reg['nchunk']) * 16:(s % reg['nchunk']) * 16 + 16] = 0
    out = conv_ref(c['mode'], pr['x'], Wm, pr['bias'], c['Ho'], c['Wo'], c['cout'], clamp=fault == 'clamp_tap')
    start = pr['out0'] if c['acc'] else torch.full_like(out, NAN)     # what the destination holds before the call
    if c['acc'] and fault != 'no_accumulate':
        out = out + pr['out0']
    if fault in ('last_strip', 'last_band', 'pad_row'):
        out = torch.where(fault_region(pr, fault), start, out)
    if fault == 'quad_shift':
        m = fault_region(pr, fault)
        out = torch.where(m, out.roll(reg['CPT'], 3), out)
    return out


def replica_sums(pr, out, drop=None):
    """the statistics workspace conv_cin12_k leaves (forward kind): workgroup (image, band, strip) adds its pixels into replica blockIdx % RV_BN_NREP.
    drop: that replica is left out (the emulated fault)."""
    c = pr['case']
    reg = case_regime(c)
    assert reg['kernel'] == 'cin12' and c['stats'] == 'sums'
    C = c['cout']
    ws = torch.zeros(RV_BN_NREP * 2 * C + SUMS_GUARD, dtype=torch.float64)
    ws[RV_BN_NREP * 2 * C:] = SUMS_MARK
    v = ws[:RV_BN_NREP * 2 * C].view(RV_BN_NREP, 2, C)
    y = out.double()
    for b in range(c['B']):
        for band in range(reg['nband']):
            for strip in range(reg['nstrip']):
                rep = ((b * reg['nband'] + band) * reg['nstrip'] + strip) % RV_BN_NREP
                if rep == drop:
                    continue
                blk = y[b, band * CIN12_ROWS:(band + 1) * CIN12_ROWS, strip * reg['PXW']:(strip + 1) * reg['PXW']].reshape(-1, C)
                v[rep, 0] += blk.sum(0)
                v[rep, 1] += (blk * blk).sum(0)
    return ws


# ---------------------------------------------------------------------------------------------------------------------
# measuring and asserting
# ---------------------------------------------------------------------------------------------------------------------
_OUT = os.path.join(os.path.dirname(parity_tol._OUT), 'conv_errors.jsonl')      # next to gemm_errors.jsonl


def check(where, case, key, ratio, log=None):
    """Assert one measured ratio error / bound (<= 1) and (log = True: on the device) append it to conv_errors.jsonl."""
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
