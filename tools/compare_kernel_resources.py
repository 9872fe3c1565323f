"""Device code of two builds of the library, kernel by kernel (CPU only; no GPU needed): registers, spills, scratch, static LDS, occupancy
from -Rpass-analysis=kernel-resource-usage and the bytes of every kernel symbol in the device ELF (profiles/product_lab_resources.txt).  For a kernel whose bytes differ it prints the differing
dwords with the two dwords in front of each (A | B).

    python tools/compare_kernel_resources.py A_DIR B_DIR [suffix_a [suffix_b]]

A_DIR / B_DIR hold, for every source x.hip, the object x<suffix>.o (suffix: '' product, '.lab', '.abl'; a missing x<suffix>.o falls back to
x.o, the object a variant shares with the product) and next to it x<suffix>.o.remarks, the stderr of its hipcc command with
-Rpass-analysis=kernel-resource-usage added (same flags otherwise: reconvat_amd/build.py FLAGS).  Kernels are matched by mangled name."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reconvat_amd import build

LLVM = os.path.join(os.path.dirname(os.path.dirname(build.HIPCC)), 'llvm', 'bin')      # the LLVM tools of the ROCm tree hipcc comes from
FIELDS = [('VGPRs', 'vgpr'), ('AGPRs', 'agpr'), ('ScratchSize [bytes/lane]', 'scratch'), ('VGPRs Spill', 'vspill'), ('SGPRs Spill', 'sspill'),
          ('LDS Size [bytes/block]', 'lds'), ('Occupancy [waves/SIMD]', 'occ')]


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def kernels_of(obj, tmp):
    """mangled name -> dict(resource figures, code = bytes of the kernel symbol)"""
    res, name = {}, None
    for line in open(obj + '.remarks'):
        m = re.search(r'remark:\s+(.*?): (\S+) \[-Rpass-analysis', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = m.group(2)
            res[name] = {}
        elif name:
            res[name][m.group(1)] = m.group(2)
    fb, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'device.co')
    run(os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fb, obj)
    run(os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--input=' + fb, '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co)
    text = None
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '-S', '--wide', co).splitlines():
        f = line.replace('[', ' ').replace(']', ' ').split()
        if len(f) > 5 and f[1] == '.text':
            text = (int(f[0]), int(f[3], 16), int(f[4], 16))          # section index, address, file offset
    blob = open(co, 'rb').read()
    out = {}
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '-s', '--wide', co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == 'FUNC' and f[6] == str(text[0]) and f[7] in res:
            off = int(f[1], 16) - text[1] + text[2]
            out[f[7]] = dict({short: res[f[7]][key] for key, short in FIELDS}, code=blob[off:off + int(f[2])])
    return out


def collect(d, suffix, tmp):
    out = {}
    for n in sorted(os.listdir(d)):
        if n.endswith('.hip'):
            base = os.path.join(d, n[:-4])
            obj = base + suffix + '.o' if os.path.exists(base + suffix + '.o') else base + '.o'
            if os.path.exists(obj):
                for k, v in kernels_of(obj, tmp).items():
                    out[(n, k)] = v
    return out


if __name__ == '__main__':
    sa, sb = (sys.argv[3:] + ['', ''])[:2]
    with tempfile.TemporaryDirectory() as tmp:
        a, b = collect(sys.argv[1], sa, tmp), collect(sys.argv[2], sb, tmp)
    both = sorted(set(a) & set(b))
    differ = [k for k in both if a[k] != b[k]]
    print(f'kernels: {len(a)} in A, {len(b)} in B, {len(both)} in both; equal in every figure and byte-identical: {len(both) - len(differ)}; differing: {len(differ)}')
    for k in differ:
        x, y = a[k]['code'], b[k]['code']
        figures = {f: (a[k][f], b[k][f]) for f in a[k] if a[k][f] != b[k][f] and f != 'code'}
        words = sorted({i // 4 * 4 for i in range(min(len(x), len(y))) if x[i] != y[i]})
        where = [f'+{w:#x}: {x[w - 8:w + 4].hex()} | {y[w - 8:w + 4].hex()}' for w in words[:2]]
        print('  DIFFERS', k[0], k[1], figures or 'all figures equal', f'code {len(x)} | {len(y)} bytes, {len(words)} dword(s) differ', *where)
    for tag, only in (('only in A', sorted(set(a) - set(b))), ('only in B', sorted(set(b) - set(a)))):
        for k in only:
            print(f'  {tag}: {k[0]} {k[1]}')
    print('\nper source: kernels in both / equal and byte-identical / sum of VGPRs / sum of code bytes (A | B)')
    for src in sorted({k[0] for k in both}):
        ks = [k for k in both if k[0] == src]
        print(f'  {src:<18} {len(ks):4d} {sum(a[k] == b[k] for k in ks):4d}   vgpr {sum(int(a[k]["vgpr"]) for k in ks)} | {sum(int(b[k]["vgpr"]) for k in ks)}'
              f'   code {sum(len(a[k]["code"]) for k in ks)} | {sum(len(b[k]["code"]) for k in ks)}')
