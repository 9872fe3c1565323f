"""Local attention, 32-frame form against the 16-frame form (reconvat_amd/csrc/attn.hip): forward and both backward kernels through
the C ABI.  Per case: (1) `out`, `att`, `dq`, `dk`, `dv`, `de` of the 32-frame form are torch.equal to the 16-frame form's in the same
build, (2) the 32-frame form stays within the operator tolerances of tests/test_ops_gpu.py of the formula in the header of attn.hip,
evaluated in fp64 on the CPU.

RV_ATTN_TILE is read once, when the library is loaded, so each form runs in a private copy of the built library loaded under its
own setting (same process, same device, same inputs).

Every tensor is an exact-size allocation, so in every case the last valid frame of the last batch is the last row of its
allocation (q, k, v, dout, att, de alike): a staging offset past the sequence end would land beyond it.  The kernels' staging is
range-checked by construction (buffer resources sized to the view); the 16-frame form and the fp64 formula would expose a row
that arrived as anything but zeros."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5        # tests/test_ops_gpu.py: forward outputs
TOL_G = 1e-4      # ... gradients
W, P = 31, 15

#        L   G  dh   fused
CASES = [(16, 2, 16, False),     # one partial tile; the window reaches past both ends of the sequence
         (33, 2, 20, False),     # a one-frame last tile; dh not a multiple of 16: pad columns
         (64, 1, 128, False),    # two full tiles; rel^T in LDS or in registers, whichever the launch code picks
         (48, 1, 229, False),    # the wide head: unaligned 16-byte rows plus the 4-byte tail, rel_regs, the single-buffer seq_kv path
         (40, 3, 16, True)]      # q/k/v as column slices of one fused [B*L, 3F] buffer: ld != F
B = 2


@pytest.fixture(scope='module')
def forms(dev, tmp_path_factory):
    """{16: library, 32: library}: two private copies of the built library, each loaded with its RV_ATTN_TILE."""
    from reconvat_amd import _lib
    _lib.load()                                   # (the build must exist and match its sources)
    d = tmp_path_factory.mktemp('attn_forms')
    libs, old = {}, os.environ.get('RV_ATTN_TILE')
    try:
        for tile in (16, 32):
            path = str(d / f'libreconvat_hip_tile{tile}.so')
            shutil.copyfile(_lib.LIB_PATH, path)
            os.environ['RV_ATTN_TILE'] = str(tile)
            lib = ctypes.CDLL(path)
            for name in ('rv_local_attn_fwd', 'rv_local_attn_bwd', 'rv_last_error'):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = _lib.SIGNATURES[name]
            libs[tile] = lib
    finally:
        if old is None:
            os.environ.pop('RV_ATTN_TILE', None)
        else:
            os.environ['RV_ATTN_TILE'] = old
    return libs


def make_inputs(L, G, dh, fused):
    g = torch.Generator().manual_seed(1000 * L + 10 * G + dh)
    F = G * dh
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    qkv = r(3, B, L, F)                                              # k, q, v (the order of the fused projection buffer)
    rel = r(F, W) * 0.5
    dout = r(B, L, F)
    return qkv, rel, dout


def reference(qkv, rel, dout, G, dh):
    """The formula of attn.hip's header in fp64: energy = q . (k window + rel), att = softmax, out = att . v window."""
    k, q, v = (t.double().requires_grad_(True) for t in qkv)
    Bq, L, F = q.shape
    win = lambda t: torch.nn.functional.pad(t, (0, 0, P, P)).unfold(1, W, 1).reshape(Bq, L, G, dh, W)   # zero padded: [B, L, G, dh, 31]
    q5 = q.reshape(Bq, L, G, dh, 1)
    energy = (q5 * (win(k) + rel.double().reshape(1, 1, G, dh, W))).sum(3)                             # [B, L, G, 31]
    energy.retain_grad()
    att = torch.softmax(energy, -1)
    out = (att.unsqueeze(3) * win(v)).sum(-1).reshape(Bq, L, F)
    (out * dout.double()).sum().backward()
    return {'out': out.detach(), 'att': att.detach(), 'dq': q.grad, 'dk': k.grad, 'dv': v.grad, 'de': energy.grad}


def run_form(lib, dev, qkv, rel, dout, G, dh, fused):
    _, Bq, L, F = qkv.shape
    st = torch.cuda.current_stream().cuda_stream
    if fused:
        buf = qkv.permute(1, 2, 0, 3).reshape(Bq * L, 3 * F).contiguous().to(dev)      # rows [k | q | v]
        k, q, v = buf[:, :F], buf[:, F:2 * F], buf[:, 2 * F:]
        ld = 3 * F
        dbuf = torch.zeros(Bq * L, 3 * F, device=dev)
        dk, dq, dv = dbuf[:, :F], dbuf[:, F:2 * F], dbuf[:, 2 * F:]
    else:
        k, q, v = (t.reshape(Bq * L, F).contiguous().to(dev) for t in qkv)
        ld = F
        dk, dq, dv = (torch.zeros(Bq * L, F, device=dev) for _ in range(3))
    relT = rel.t().contiguous().to(dev)                                                # [31, F]
    do = dout.contiguous().to(dev)
    out = torch.zeros(Bq, L, F, device=dev)
    att = torch.zeros(Bq, L, G, W, device=dev)
    de = torch.zeros(Bq, L, G, W, device=dev)
    p = lambda t: t.data_ptr()
    rc = lib.rv_local_attn_fwd(p(q), p(k), p(v), ld, p(relT), p(out), p(att), Bq, L, G, dh, st)
    assert rc == 0, lib.rv_last_error().decode()
    rc = lib.rv_local_attn_bwd(p(do), p(q), p(k), p(v), ld, p(relT), p(att), p(dq), p(dk), p(dv), ld, p(de), Bq, L, G, dh, st)
    assert rc == 0, lib.rv_last_error().decode()
    torch.cuda.synchronize()
    return {'out': out.cpu(), 'att': att.cpu(), 'dq': dq.cpu().reshape(Bq, L, F), 'dk': dk.cpu().reshape(Bq, L, F),
            'dv': dv.cpu().reshape(Bq, L, F), 'de': de.cpu()}


@pytest.mark.parametrize('L,G,dh,fused', CASES)
def test_tile32_matches_tile16_and_formula(dev, forms, L, G, dh, fused):
    qkv, rel, dout = make_inputs(L, G, dh, fused)
    assert all(torch.isfinite(t).all() for t in (qkv, rel, dout))
    r16 = run_form(forms[16], dev, qkv, rel, dout, G, dh, fused)
    r32 = run_form(forms[32], dev, qkv, rel, dout, G, dh, fused)
    ref = reference(qkv, rel, dout, G, dh)
    errs = {n: rel_err(r32[n], ref[n]) for n in ref}
    print(f'L={L} G={G} dh={dh} fused={fused}: 32-frame form against the fp64 formula', {n: f'{e:.1e}' for n, e in errs.items()},
          '| bit-equal to the 16-frame form:', {n: torch.equal(r32[n], r16[n]) for n in ref})
    for n in ref:
        assert torch.equal(r32[n], r16[n]), f'{n}: the 32-frame form differs from the 16-frame form'
    for n in ('out', 'att'):
        assert errs[n] < TOL, (n, errs[n])
    for n in ('dq', 'dk', 'dv', 'de'):
        assert errs[n] < TOL_G, (n, errs[n])


def test_buffer_lds_dma_takes_unaligned_views_and_negative_offsets(tmp_path):
    """What stage_rows_buf relies on beyond tests/test_probes_gpu.py: 16-byte buffer DMA lanes on a view that is only 4-byte aligned
    (229-float rows), and byte offsets in front of the view (rows before the sequence start) count as out of range: zeros."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path / 'buffer_lds16_unaligned')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O2', os.path.join(root, 'tools', 'probes', 'buffer_lds16_unaligned.hip'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(': ok') == 8, r.stdout
