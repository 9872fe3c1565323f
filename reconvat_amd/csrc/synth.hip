// Additive synthesiser: renders a table of partial rows to audio, so that a note list becomes a waveform on the device.
// reconvat_amd/synth.py has the definition; in short, a row is eight 32-bit words
//     s, e (int)  inc, ph (uint32, 2^-32 turn)  amp, dec (float32)  A, R (int)
// and contributes, with t = n - s and for s <= n < e + R,
//     amp * min(t + 1, A) / A * exp(-dec t) * (n < e ? 1 : ((e + R - n) / R)^2) * sin(2 pi ((ph + inc t) mod 2^32) / 2^32).
// y[n] is the sum over the rows in ascending row order.
//
// One workgroup of 256 work items owns one tile of SYN_TILE = 1024 ABSOLUTE samples [1024 j, 1024 (j + 1)), four consecutive samples
// per work item, so a wave owns 256 consecutive samples.  The host hands over, per tile, the ascending list of the rows that meet
// it (CSR: tile_ptr, tile_rows).  The list index is wave-uniform: the row number and the row's eight words arrive by scalar loads,
// and a wave skips a row that misses its 256 samples with a scalar branch.  Per term, in float32: theta in exact uint32 arithmetic,
// read as a SIGNED count of 2^-31 half-turns and handed to sinpif (so the conversion to float costs 2^-26 turn at most, not 2^-25),
// expf of one rounded product, one correctly rounded division for each envelope factor, four products -- and one add into a
// float64 accumulator, so the error does not grow with the number of rows that sound at once.  No recurrences: sine and exponential
// are evaluated afresh for every sample.  The tiles are absolute and the order is the list's: the bits of an output depend neither
// on n0 nor on n_out nor on where a caller cuts a long render into calls.  No LDS, no atomics, no allocation, no synchronisation.
#include "common.h"

#define SYN_TILE 1024
#define SYN_MAX_TILES ((1 << 21) - 1)          // every sample index stays below 2^31 - 1024

struct SynthArgs {
    const unsigned* rows; const int* tile_ptr; const int* tile_rows;
    void* y;
    long n0, n_out;
    int n_rows, tile0;
};

template <bool OUT_I16> __global__ __launch_bounds__(256) void synth_render_k(SynthArgs a) {
    const unsigned* __restrict__ rows = a.rows;
    const int* __restrict__ tile_rows = a.tile_rows;
    const int tile = a.tile0 + (int)blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w0 = tile * SYN_TILE + wave * 256;                       // the wave's first sample
    const int nb = tile * SYN_TILE + (int)threadIdx.x * 4;              // the work item's first sample
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int p0 = a.tile_ptr[tile], p1 = a.tile_ptr[tile + 1];
    for (int p = p0; p < p1; ++p) {
        const int r = tile_rows[p];
        if (r < 0 || r >= a.n_rows) continue;                          // an entry outside the table is skipped
        const unsigned* row = rows + (long)r * 8;
        const int s = (int)row[0], e = (int)row[1];
        const unsigned inc = row[2], ph = row[3];
        const float amp = __uint_as_float(row[4]), dec = __uint_as_float(row[5]);
        const int A = (int)row[6], R = (int)row[7];
        const long end64 = (long)e + (long)R;                          // one past the last sample of the row
        if ((long)s >= (long)w0 + 256 || end64 <= (long)w0) continue;   // the row misses this wave's samples
        const int end = end64 > 0x7fffffffL ? 0x7fffffff : (int)end64; // every n is below 2^31 - 1024: the clamp moves no `on`
        const unsigned endu = (unsigned)end64;                         // end - n below: in (0, R] wherever it is used, exact mod 2^32
        const float fA = (float)A, fR = (float)R;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = nb + i;
            const bool on = n >= s && n < end;
            const unsigned t = (unsigned)n - (unsigned)s;              // exact wherever the row sounds
            const unsigned ta = t + 1u < (unsigned)A ? t + 1u : (unsigned)A;
            const float att = __fdiv_rn((float)ta, fA);
            const float q = __fdiv_rn((float)(endu - (unsigned)n), fR);
            const float rel = n < e ? 1.0f : __fmul_rn(q, q);
            const float decay = expf(-__fmul_rn(dec, (float)t));
            const unsigned theta = ph + inc * t;
            const float osc = sinpif(__fmul_rn((float)(int)theta, 4.656612873077392578125e-10f));      // 2^-31: exact scaling
            const float v = __fmul_rn(__fmul_rn(__fmul_rn(__fmul_rn(amp, att), decay), rel), osc);
            acc[i] += on ? (double)v : 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long o = (long)(nb + i) - a.n0;
        if (o >= 0 && o < a.n_out) {
            if (OUT_I16) {
                const double v = fmin(fmax(rint(acc[i] * 32768.0), -32768.0), 32767.0);      // round half to even, saturate
                reinterpret_cast<short*>(a.y)[o] = (short)(int)v;
            } else {
                reinterpret_cast<float*>(a.y)[o] = (float)acc[i];
            }
        }
    }
}

extern "C" {

// rows [n_rows][8] as above; tile_ptr [n_tiles + 1], tile_rows [tile_ptr[n_tiles]]: tile j lists, in ascending order, the rows whose
// [s, e + R) meets [1024 j, 1024 (j + 1)).  y: n_out samples of out_dtype (0 float32, 1 int16 = saturated round-half-even of 32768 y);
// y[0] is sample n0.
int rv_synth_render(const unsigned* rows, int n_rows, const int* tile_ptr, const int* tile_rows, int n_tiles, long n0, long n_out,
                    void* y, int out_dtype, void* stream) {
    RV_CHECK_ARG(tile_ptr && y, "rv_synth_render: null pointer");
    RV_CHECK_ARG(n_rows >= 0 && (n_rows == 0 || rows), "rv_synth_render: %d rows and no table", n_rows);
    RV_CHECK_ARG(n_tiles >= 0 && n_tiles <= SYN_MAX_TILES, "rv_synth_render: n_tiles %d outside [0, %d]", n_tiles, SYN_MAX_TILES);
    RV_CHECK_ARG(out_dtype == 0 || out_dtype == 1, "rv_synth_render: unknown sample type %d", out_dtype);
    RV_CHECK_ARG(n0 >= 0 && n_out >= 0 && n0 <= (long)n_tiles * SYN_TILE && n_out <= (long)n_tiles * SYN_TILE - n0,
                 "rv_synth_render: samples [%ld, %ld + %ld) reach outside the %d tiles of the table", n0, n0, n_out, n_tiles);
    if (n_out == 0) return RV_OK;
    SynthArgs a;
    a.rows = rows; a.tile_ptr = tile_ptr; a.tile_rows = tile_rows; a.y = y; a.n0 = n0; a.n_out = n_out; a.n_rows = n_rows;
    a.tile0 = (int)(n0 / SYN_TILE);
    const unsigned grid = (unsigned)((n0 + n_out - 1) / SYN_TILE - a.tile0 + 1);
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == 1) hipLaunchKernelGGL((synth_render_k<true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((synth_render_k<false>), dim3(grid), dim3(256), 0, st, a);
    RV_LAUNCH_CHECK("rv_synth_render");
    return RV_OK;
}

}  // extern "C"
