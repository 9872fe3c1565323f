"""Build libreconvat_hip.so (gfx950 only) in-tree with hipcc.  No JIT cache: the .so lives next to the
sources so it travels with the repo snapshot to the GPU box.

Three variants (csrc/common.h, RV_KNOB).  `product` is the library the package loads and the only one build() makes by default: it reads
no experiment knob from the environment.  `lab` adds the host-side knobs and the prototypes of tools/; `ablation` adds the in-kernel
timing hooks on top (WRONG results by design).  The two are for tools/ only and load through RECONVAT_HIP_LIB=<path>."""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libreconvat_hip.so')
SOURCES = ['conv.hip', 'conv_wino2.hip', 'bn.hip', 'gemm.hip', 'attn.hip', 'elementwise.hip', 'mel.hip', 'cqt.hip', 'thickstun.hip', 'data.hip', 'acoustics.hip', 'resample.hip', 'synth.hip', 'align.hip', 'eval.hip', 'velocity.hip', 'hmm.hip', 'onset_time.hip', 'lstm.hip', 'api.cpp']
# the sources whose host code changes with the variant (RV_KNOB / RV_LAB / RV_ABLATION; tests/test_abi.py checks the list): a variant
# compiles these and LAB_SOURCES to objects of its own and shares every other object with the product
VARIANT_SOURCES = ['conv.hip', 'conv_wino2.hip', 'bn.hip']
LAB_SOURCES = ['gemm_bf16x6.hip']            # prototypes with a negative result: in no product library
# variant -> (library suffix, object suffix, flags)
VARIANTS = {'product': ('', '', []), 'lab': ('_lab', '.lab', ['-DRV_LAB']), 'ablation': ('_abl', '.abl', ['-DRV_ABLATION'])}
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function']


def source_digest():
    """sha256 (first 16 hex digits) over every kernel / ABI source in csrc/ (names and contents, sorted): baked into the library as
    rv_source_digest() and compared by reconvat_amd._lib.load() with the sources that travelled next to the .so."""
    h = hashlib.sha256()
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h', '.cpp')):
            h.update(name.encode() + b'\0')
            with open(os.path.join(CSRC, name), 'rb') as fh:
                h.update(fh.read())
            h.update(b'\0')
    return h.hexdigest()[:16]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def object_path(src, variant):
    own = src in VARIANT_SOURCES + LAB_SOURCES         # every other source is the same text in every variant: the product's object
    return os.path.join(CSRC, os.path.splitext(src)[0] + (VARIANTS[variant][1] if own else '') + '.o')


def _compile(src, variant='product'):
    obj = object_path(src, variant)
    vflags = VARIANTS[variant][2] if src in VARIANT_SOURCES + LAB_SOURCES else []
    path = os.path.join(CSRC, src)
    deps = [path] + [os.path.join(CSRC, n) for n in sorted(os.listdir(CSRC)) if n.endswith('.h')]
    extra, stale = list(vflags), _stale(obj, deps)
    if src == 'api.cpp':                       # carries the digest of ALL sources: rebuilt whenever any of them changed
        dig = source_digest()
        extra = [f'-DRV_SOURCE_DIGEST="{dig}"']
        side = obj + '.digest'
        stale = stale or not os.path.exists(side) or open(side).read().strip() != dig
    if stale:
        cmd = [HIPCC] + FLAGS + extra + (['-x', 'hip'] if src.endswith('.cpp') else []) + ['-c', path, '-o', obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'hipcc failed for {src}:\n{r.stderr}')
        if r.stderr.strip():
            sys.stderr.write(r.stderr)
        if src == 'api.cpp':
            with open(obj + '.digest', 'w') as fh:
                fh.write(dig)
    return obj


def lib_path(variant='product'):
    return os.path.join(HERE, f'libreconvat_hip{VARIANTS[variant][0]}.so')


def build(force=False, verbose=False, variant='product'):
    sources = SOURCES + (LAB_SOURCES if variant != 'product' else [])
    if force:
        for s in sources:
            if os.path.exists(object_path(s, variant)):
                os.remove(object_path(s, variant))
    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(lambda s: _compile(s, variant), sources))
    lib = lib_path(variant)
    if force or _stale(lib, objs):
        cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC'] + objs + ['-o', lib]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'link failed:\n{r.stderr}')
    if verbose:
        print('built', lib)
    return lib


if __name__ == '__main__':
    build(force='--force' in sys.argv, verbose=True,
          variant='ablation' if '--ablation' in sys.argv else 'lab' if '--lab' in sys.argv else 'product')
