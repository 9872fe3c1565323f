// The host-side band plan of the persistent 3x3 band kernels: conv3x3_lds_k and conv3x3_wino_k (conv.hip), conv3x3_wino2_k
// (conv_wino2.hip) -- the persistent grid and the ONE Winograd band plan.  Nothing of the device side is here: moved into functions, the band
// epilogue and the statistics fold change the kernels' register allocation and the Winograd prologue their code
// (profiles/band_epilogue_resources.txt), so each kernel keeps its copy.
#pragma once
#include "conv_shared.h"

// Persistent grid of a band kernel (aa.TH set): wg_slots workgroup slots on the chip shared by the n-splits, every workgroup a run of
// bands_per_wg bands.  Returns the number of workgroups.
static inline unsigned band_grid(ConvLdsArgs& aa, int NT, int wg_slots) {
    aa.nbands = cdiv(aa.c.H, aa.TH);
    aa.total_bands = aa.c.B * aa.nbands;
    const int nsplit = aa.c.ntile_n / NT;
    int wgs = wg_slots / nsplit;
    if (wgs < 1) wgs = 1;
    if (wgs > aa.total_bands) wgs = aa.total_bands;
    aa.bands_per_wg = cdiv(aa.total_bands, wgs);
    wgs = cdiv(aa.total_bands, aa.bands_per_wg);
    aa.nsplit = nsplit; aa.xcd = 1;      // XCD-aware placement: worth 0.35 ms per step; the kernels' xcd == 0 branch is unreachable
    return (unsigned)(wgs * nsplit);
}

// LDS bytes of a Winograd band kernel: two band buffers of TH + 2 rows of 1 KiB pieces (16 pixels x 16 channels), wslots chunks of weights
static inline size_t wino_band_bytes(int NT, int TH, int W, int wslots) {
    const int NP = (2 * ((W + 1) / 2) + 2 + 15) / 16;
    return (size_t)2 * (TH + 2) * NP * 1024 + (size_t)wslots * 16 * NT * 1024;
}

// Where the weights of a Winograd band kernel live.  They travel through `ring` chunk slots (conv3x3_wino_k: 2, the band's double
// buffer; conv3x3_wino2_k: 3, the chunk of unit u is still being read while unit u + 2 is on its way) unless all chunks fit next to the
// two band buffers and may stay resident (no weight DMA after the first band, 16 NT KiB less L2 traffic per unit).  ring_is_resident:
// nchunk <= ring already counts as resident (the pipelined kernel then addresses the slots by chunk).
struct WinoWeightPolicy {
    int ring;
    bool ring_is_resident, try_resident;
};

// Band plan of a Winograd kernel of nw waves with MTW tile groups per wave: a band of TH (even) rows holds (TH/2) x ceil(W/2) tiles of
// 2x2 outputs, nw x MTW groups of 16 tiles per unit.  force_th = 0: as many rows as the tile slots and the LDS (cap bytes) hold -- a
// staged row is a whole number of 1 KiB pieces, so e.g. a 114-pixel row takes 8 KiB.  Fills aa (ablate = 0), the grid and the LDS bytes.
static inline int wino_band_plan(ConvLdsArgs& aa, dim3& grid, size_t& lds, const ConvArgs& a0, int NT, int MTW, int nw, int force_th,
                                 size_t cap, int wg_slots, const WinoWeightPolicy wp) {
    if (NT < 1 || a0.ntile_n % NT) return RV_EUNSUPPORTED;
    if (nw == 12 && a0.bn_z) return RV_EUNSUPPORTED;      // three waves per SIMD: the fused BatchNorm-backward epilogue does not fit without scratch
    aa.c = a0;
    const long in_bytes = (((long)a0.B * a0.H * a0.W - 1) * a0.in_ld + a0.Cin) * 4;
    if (in_bytes >= 0x3f000000L) return RV_EUNSUPPORTED;      // the staging loads address the input view with 30-bit offsets (see the kernels)
    aa.in_bytes = (unsigned)in_bytes;
    const int WT = (a0.W + 1) / 2;
    aa.c.fd_pw = fastdiv_make((unsigned)WT);
    const int trows = (nw * MTW * 16) / WT;
    if (trows < 1) return RV_EUNSUPPORTED;
    int TH = 2 * trows;
    if (TH > a0.H) TH = (a0.H + 1) & ~1;
    if (force_th) {
        if (force_th > TH || (force_th & 1)) return RV_EUNSUPPORTED;
        TH = force_th;
    }
    const int ring = a0.nchunk < wp.ring ? a0.nchunk : wp.ring;
    lds = wino_band_bytes(NT, TH, a0.W, ring);
    while (!force_th && lds > cap && TH > 2) {
        TH -= 2;
        lds = wino_band_bytes(NT, TH, a0.W, ring);
    }
    aa.wres = (wp.ring_is_resident && a0.nchunk <= wp.ring) ? 1 : 0;
    if (!aa.wres && a0.nchunk > 1 && wp.try_resident) {
        const size_t lds_res = wino_band_bytes(NT, TH, a0.W, a0.nchunk);
        if (lds_res <= cap) { aa.wres = 1; lds = lds_res; }
    }
    if (lds > cap) return RV_EUNSUPPORTED;
    aa.TH = TH;
    grid = dim3(band_grid(aa, NT, wg_slots));
    aa.nbuf = 2; aa.skew = 0; aa.ablate = 0;
    return RV_OK;
}
