// Probe: does `buffer_load_dwordx4 ... offen lds` accept a source (resource base + offset) that is only 4-byte aligned, and does a
// negative byte offset (it wraps to >= 0xC0000000) count as out of range, i.e. write zeros?
//   hipcc --offload-arch=gfx950 -O2 tools/probes/buffer_lds16_unaligned.hip -o tools/probes/buffer_lds16_unaligned && tools/probes/buffer_lds16_unaligned
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
__global__ void k(const float* in, float* out, int shift, unsigned bytes, int neg) {
    __shared__ __attribute__((aligned(16))) float smem[256];
    for (int q = 0; q < 4; ++q) smem[threadIdx.x * 4 + q] = -7.f;
    __syncthreads();
    auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(in + shift), 0, bytes, 0x00020000);   // base 4-byte aligned only when shift % 4 != 0
    unsigned voff = threadIdx.x * 16u;
    if (neg && threadIdx.x >= 32) voff = (unsigned)(-(int)(threadIdx.x * 16u));               // lanes 32..63: in front of the view
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)smem, 16, voff, 0, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int q = 0; q < 4; ++q) out[threadIdx.x * 4 + q] = smem[threadIdx.x * 4 + q];
}
int main() {
    const int n = 2048;
    std::vector<float> h(n);
    for (int i = 0; i < n; ++i) h[i] = 1.f + i;
    float *d, *o;
    (void)hipMalloc(&d, n * 4); (void)hipMalloc(&o, 256 * 4);
    (void)hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice);
    int rc = 0;
    for (int neg = 0; neg < 2; ++neg)
        for (int shift = 0; shift < 4; ++shift) {
            // the view starts 1024 floats into the allocation, so a negative offset that was NOT range-checked would read valid memory
            hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d + 1024, o, shift, 256 * 4u, neg);
            std::vector<float> r(256);
            (void)hipMemcpy(r.data(), o, 256 * 4, hipMemcpyDeviceToHost);
            int bad = 0;
            for (int i = 0; i < 256; ++i) {
                const float want = (neg && i >= 128) ? 0.f : 1.f + 1024 + shift + i;
                if (r[i] != want) { if (bad < 4) printf("shift %d neg %d elem %d: got %g want %g\n", shift, neg, i, r[i], want); ++bad; }
            }
            printf("buffer_load_dwordx4 lds, view shifted by %d floats%s: %s\n", shift, neg ? ", lanes 32..63 at negative offsets" : "", bad ? "WRONG" : "ok");
            rc |= bad != 0;
        }
    return rc;
}
