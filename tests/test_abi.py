"""CPU checks of the drop-in boundary: the shared library loads, exports every symbol that
include/reconvat_hip.h declares, and the ctypes prototypes agree with the header (argument counts and C type classes);
the product library carries no lab code and reads the environment in attn.hip only (reconvat_amd/build.py: variants).
No compute call is made (there is no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_class(decl, named):
    """Type class of a C parameter (`named`: the declaration ends in the parameter's name) or return type."""
    if '*' in decl:
        return 'pointer'
    words = [w for w in decl.split() if w != 'const']
    if named:
        words = words[:-1]
    return {('int',): 'int', ('unsigned',): 'unsigned', ('unsigned', 'int'): 'unsigned', ('long',): 'long', ('float',): 'float'}[tuple(words)]


CTYPES_CLASS = {ctypes.c_int: 'int', ctypes.c_uint: 'unsigned', ctypes.c_long: 'long', ctypes.c_float: 'float',
                ctypes.c_void_p: 'pointer', ctypes.c_char_p: 'pointer'}


def header_decls():
    """name -> (class of the return value, [class of every argument]); classes: int, unsigned, long, float, pointer"""
    text = open(os.path.join(ROOT, 'include', 'reconvat_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decls = {}
    for m in re.finditer(r'\b(int|long|const char\*)\s+(rv_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S):
        args = m.group(3).strip()
        args = [] if args in ('', 'void') else [a for a in args.split(',') if a.strip()]
        decls[m.group(2)] = (c_class(m.group(1), False), [c_class(a, True) for a in args])
    return decls


@pytest.fixture(scope='module')
def built():
    from reconvat_amd import build
    return build.build()


def test_header_symbols_exported(built):
    lib = ctypes.CDLL(built)
    decls = header_decls()
    assert len(decls) >= 20
    for name in decls:
        assert hasattr(lib, name), f'{name} declared in include/reconvat_hip.h but not exported'


def test_ctypes_signatures_match_header(built):
    from reconvat_amd import _lib
    decls = header_decls()
    assert set(decls) == set(_lib.SIGNATURES), set(decls) ^ set(_lib.SIGNATURES)
    for name, (ret, args) in decls.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(args), name
        assert [CTYPES_CLASS[t] for t in argtypes] == args, name
        assert CTYPES_CLASS[restype] == ret, name
    lib = _lib.load()
    assert lib.rv_abi_version() == 1
    # the library records the sources it was built from; load() refuses a library built from other sources (next test)
    assert lib.rv_source_digest().decode() == _lib.source_digest() and len(_lib.source_digest()) == 16
    assert lib.rv_packed_weight_floats(9, 16, 16) == (9 + 16) * 1 * 1 * 64 * 4      # nine tap fragments + the 16 Winograd fragments
    assert lib.rv_packed_weight_floats(9, 8, 16) == 9 * 1 * 1 * 64 * 2
    assert lib.rv_packed_weight_floats(9, 1, 16) == 9 * 16
    assert lib.rv_reduce_workspace_bytes(4096) == 8


def undefined_symbols(obj):
    from reconvat_amd import build
    readelf = os.path.join(os.path.dirname(os.path.dirname(build.HIPCC)), 'llvm', 'bin', 'llvm-readelf')
    out = subprocess.run([readelf, '-s', '--wide', obj], capture_output=True, text=True, check=True).stdout
    return {f[7].split('@')[0] for f in (line.split() for line in out.splitlines()) if len(f) == 8 and f[6] == 'UND'}


def test_product_reads_the_environment_in_attn_only(built):
    """No launch path of the product library calls getenv: the experiment knobs are RV_KNOB (csrc/common.h), literals outside the lab
    builds.  attn.hip reads RV_ATTN_TILE[_WIDE] / RV_ATTN_WAVES[_WIDE] once, when the library is loaded (tests/test_attn_tiles_gpu.py)."""
    from reconvat_amd import build
    assert 'getenv' in undefined_symbols(build.object_path('attn.hip', 'product'))      # (the reader finds the symbol where it is)
    for src in build.SOURCES:
        if src != 'attn.hip':
            assert 'getenv' not in undefined_symbols(build.object_path(src, 'product')), src


def test_product_has_no_lab_code(built):
    from reconvat_amd import build
    lib = ctypes.CDLL(built)
    assert built == build.lib_path('product') and os.path.basename(built) == 'libreconvat_hip.so'
    for name in ('rv_debug_mfma_peak', 'rv_debug_gemm_bf16x6'):
        assert not hasattr(lib, name), f'{name}: a lab prototype in the product library'
    assert not set(build.LAB_SOURCES) & set(build.SOURCES)
    # the sources a variant compiles for itself are exactly those that name a variant macro (the headers are included by them)
    names = {n for n in os.listdir(build.CSRC) if n.endswith(('.hip', '.cpp'))
             and re.search(r'\bRV_(KNOB|LAB|ABLATION|ABLATE_MASK)\b|\brv_dbg_ptr\b', open(os.path.join(build.CSRC, n)).read())}
    assert names == set(build.VARIANT_SOURCES), names


@pytest.mark.parametrize('variant', ['lab', 'ablation'])
def test_variant_host_code_compiles(variant):
    """The lab and ablation variants are built by hand, for tools/ only: the host pass (syntax only, seconds) of the sources they compile
    for themselves keeps their knob code from rotting.  A full variant build is minutes of device compilation and is not a test."""
    from reconvat_amd import build
    for src in build.VARIANT_SOURCES + build.LAB_SOURCES:
        cmd = [build.HIPCC] + build.FLAGS + build.VARIANTS[variant][2] + ['--cuda-host-only', '-fsyntax-only', os.path.join(build.CSRC, src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, f'{src} ({variant}):\n{r.stderr}'


def test_stale_library_is_refused(built, monkeypatch):
    """A prebuilt .so whose baked-in source digest differs from the sources next to it must not load (the library is
    git-ignored and ships prebuilt; nothing else ties it to the sources)."""
    from reconvat_amd import _lib, build
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(build, 'source_digest', lambda: '0123456789abcdef')
    monkeypatch.delenv('RECONVAT_HIP_LIB', raising=False)
    monkeypatch.delenv('RV_SKIP_DIGEST_CHECK', raising=False)
    with pytest.raises(RuntimeError, match='rebuild it'):
        _lib.load()


def test_no_cpu_fallback():
    """The product path must fail loudly on CPU tensors -- never route through PyTorch/the oracle."""
    import torch
    from reconvat_amd import ops, UNet_Onset
    x = torch.zeros(1, 4, 4, 16)
    w = torch.zeros(16, 16, 3, 3)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ops.ConvFn.apply(x, w, None, 'c3', None)
    m = UNet_Onset((2, 2), (2, 2), log=True, reconstruction=False, mode='imagewise', spec='Mel')
    batch = {'audio': torch.zeros(1, 32768), 'onset': torch.zeros(1, 64, 88), 'frame': torch.zeros(1, 64, 88)}
    with pytest.raises(RuntimeError, match='HIP device only'):
        m.run_on_batch(batch, None, False)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'reconvat_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f
