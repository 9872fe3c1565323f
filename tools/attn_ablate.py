"""rv_local_attn_fwd alone (B = 8, L = 640; the two head shapes of the step) under the library RECONVAT_HIP_LIB points at -- one line per run; used by
tools/attn_ablate.sh with the -DRV_ATTN_ABL=mask builds (mask: 1 no staging, 2 no score MFMAs, 4 no softmax, 8 no banded apply, 16 return at entry).

    python tools/attn_ablate.py --ladder [parent.so]
times the whole ladder in ONE process for the 16-frame form and the 32-frame form at 5 and 10 waves: every (mask, form) pair is a private copy
of reconvat_amd/libreconvat_hip_attn<mask>.so loaded under its own RV_ATTN_TILE / RV_ATTN_WAVES (they are read when a library is loaded); with a
second argument that library (the parent commit's build) is timed too, as the `parent` column of mask 0."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from reconvat_amd import _lib

ladder = len(sys.argv) > 1 and sys.argv[1] == '--ladder'
mask = int(sys.argv[1]) if len(sys.argv) > 1 and not ladder else 0
names = {0: 'full kernel', 16: 'return at entry (launch floor)', 1: 'no staging', 3: 'no staging, no scores', 7: 'no staging / scores / softmax',
         15: 'everything off (skeleton + barriers)', 2: 'no score MFMAs', 4: 'no softmax', 8: 'no banded apply'}
dev = torch.device('cuda:0')
st = torch.cuda.current_stream()


def time_shapes(lib):
    out = []
    for g, dh in ((6, 128), (4, 229)):
        f = g * dh
        qkv = torch.rand(8 * 640, 3 * f, device=dev) - 0.5
        rel = torch.rand(31, f, device=dev) - 0.5
        o = torch.empty(8, 640, f, device=dev)
        att = torch.empty(8, 640, g, 31, device=dev)
        args = (qkv.data_ptr(), qkv.data_ptr() + 4 * f, qkv.data_ptr() + 8 * f, 3 * f, rel.data_ptr(), o.data_ptr(), att.data_ptr(), 8, 640, g, dh, st.cuda_stream)
        for _ in range(3):
            assert lib.rv_local_attn_fwd(*args) == 0
        best = None
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(10):
                lib.rv_local_attn_fwd(*args)
            e1.record(st)
            e1.synchronize()
            t = e0.elapsed_time(e1) / 10 * 1e3
            best = t if best is None else min(best, t)
        out.append(f'G={g} dh={dh}: {best:6.1f} us')
    return out


if not ladder:
    print(f'mask {mask:>2} {names.get(mask, ""):<40} ' + '   '.join(time_shapes(_lib.load())))
else:
    import ctypes
    import shutil
    import tempfile
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tempfile.mkdtemp()

    def private(path, tag, env):
        for k in ('RV_ATTN_TILE', 'RV_ATTN_WAVES', 'RV_ATTN_TILE_WIDE', 'RV_ATTN_WAVES_WIDE'):
            os.environ.pop(k, None)
        os.environ.update(env)
        copy = os.path.join(tmp, tag + '.so')
        shutil.copyfile(path, copy)
        lib = ctypes.CDLL(copy)
        lib.rv_local_attn_fwd.restype, lib.rv_local_attn_fwd.argtypes = _lib.SIGNATURES['rv_local_attn_fwd']
        return lib
    forms = (('16 frames', {'RV_ATTN_TILE': '16'}), ('32 x 5 waves', {'RV_ATTN_TILE': '32', 'RV_ATTN_WAVES': '5'}),
             ('32 x 10 waves', {'RV_ATTN_TILE': '32', 'RV_ATTN_WAVES': '10'}))
    if len(sys.argv) > 2:
        print(f'parent build, full kernel: ' + '   '.join(time_shapes(private(sys.argv[2], 'parent', {}))), flush=True)
    for m in (0, 16, 1, 3, 7, 15, 2, 4, 8):
        for fi, (fname, env) in enumerate(forms):
            lib = private(os.path.join(here, 'reconvat_amd', f'libreconvat_hip_attn{m}.so'), f'm{m}_{fi}', env)
            print(f'mask {m:>2} {names.get(m, ""):<40} {fname:<14} ' + '   '.join(time_shapes(lib)), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
