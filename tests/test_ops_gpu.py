"""GPU parity of every HIP operator against a plain PyTorch fp32 CPU reference of the same op.
Tolerances are relative to the reference tensor's max magnitude (fp32 accumulation-order noise)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
TOL_G = 1e-4


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


CONV_CASES = [
    # kind, cin, cout, H, W
    ('c3', 1, 16, 9, 21), ('c3', 16, 16, 9, 21), ('c3', 16, 32, 8, 14), ('c3', 32, 32, 8, 14),
    ('c3', 32, 64, 6, 7), ('c3', 64, 64, 6, 7), ('c3', 64, 128, 5, 6), ('c3', 128, 128, 5, 6),
    ('t3', 192, 96, 5, 6), ('t3', 96, 64, 5, 6), ('t3', 96, 48, 6, 9), ('t3', 48, 32, 6, 9),
    ('t3', 48, 24, 8, 13), ('t3', 24, 16, 8, 13), ('t3', 16, 8, 9, 21), ('t3', 8, 2, 9, 21), ('t3', 8, 1, 9, 21),
    ('c1', 1, 16, 9, 21), ('c1', 16, 32, 8, 14), ('c1', 32, 64, 6, 7), ('c1', 64, 128, 5, 6),
    ('down', 16, 16, 9, 21), ('down', 32, 32, 8, 14), ('down', 64, 64, 6, 7), ('down', 128, 128, 4, 6),
    ('up', 128, 128, 3, 4), ('up', 64, 64, 4, 6), ('up', 32, 32, 5, 7), ('up', 16, 16, 6, 9),
]


def torch_conv(kind, x, w, b, size=None):
    if kind == 'c3':
        return F.conv2d(x, w, b, padding=1)
    if kind == 't3':
        return F.conv_transpose2d(x, w, b, padding=1)
    if kind == 'c1':
        return F.conv2d(x, w, b)
    if kind == 'down':
        return F.conv2d(x, w, b, stride=2)
    op = (size[0] - 2 * x.shape[2], size[1] - 2 * x.shape[3])
    return F.conv_transpose2d(x, w, b, stride=2, output_padding=op)


@pytest.mark.parametrize('kind,cin,cout,H,W', CONV_CASES)
def test_conv_fwd_bwd(dev, kind, cin, cout, H, W):
    from reconvat_amd import ops
    B = 2
    wshape = {'c3': (cout, cin, 3, 3), 't3': (cin, cout, 3, 3), 'c1': (cout, cin, 1, 1), 'down': (cout, cin, 2, 2),
              'up': (cin, cout, 2, 2)}[kind]
    x = rnd(B, cin, H, W, seed=1)
    w = rnd(*wshape, seed=2, scale=0.3)
    b = rnd(cout, seed=3)
    sizes = [None]
    if kind == 'up':
        sizes = [(2 * H, 2 * W), (2 * H, 2 * W + 1), (2 * H + 1, 2 * W + 1)]
    for size in sizes:
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yr = torch_conv(kind, xr, wr, br, size)
        cot = rnd(*yr.shape, seed=4)
        (yr * cot).sum().backward()
        xg = nhwc(x).to(dev).requires_grad_(True)
        wg = w.to(dev).requires_grad_(True)
        bg = b.to(dev).requires_grad_(True)
        ops.invalidate_weight_cache()
        yg = ops.ConvFn.apply(xg, wg, bg, kind, size)
        (yg * nhwc(cot).to(dev)).sum().backward()
        assert rel_err(nchw(yg), yr) < TOL, 'fwd'
        assert rel_err(nchw(xg.grad), xr.grad) < TOL_G, 'dgrad'
        assert rel_err(wg.grad, wr.grad) < TOL_G, 'wgrad'
        assert rel_err(bg.grad, br.grad) < TOL_G, 'bias grad'


def test_conv_large_tiles(dev):
    """Enough pixels that the (NT, MT) heuristic picks the big tiles, with a ragged tail."""
    from reconvat_amd import ops
    for kind, cin, cout, H, W in (('c3', 16, 16, 97, 229), ('c3', 64, 64, 40, 57), ('t3', 48, 24, 60, 114)):
        x = rnd(2, cin, H, W, seed=5)
        w = rnd(*((cout, cin, 3, 3) if kind == 'c3' else (cin, cout, 3, 3)), seed=6, scale=0.2)
        b = rnd(cout, seed=7)
        yr = torch_conv(kind, x, w, b)
        yg = ops.ConvFn.apply(nhwc(x).to(dev), w.to(dev), b.to(dev), kind, None)
        assert rel_err(nchw(yg), yr) < TOL


def test_upcat(dev):
    from reconvat_amd import ops
    B, H, W = 2, 5, 7
    x = rnd(B, 32, H, W, seed=1)
    s = rnd(B, 16, 2 * H, 2 * W + 1, seed=2)
    wu, bu = rnd(32, 32, 2, 2, seed=3, scale=0.3), rnd(32, seed=4)
    ws, bs = rnd(16, 16, 3, 3, seed=5, scale=0.3), rnd(16, seed=6)
    leaves = [t.clone().requires_grad_(True) for t in (x, wu, bu, s, ws, bs)]
    size = (2 * H, 2 * W + 1)
    ref = torch.cat((torch_conv('up', leaves[0], leaves[1], leaves[2], size), F.conv2d(leaves[3], leaves[4], leaves[5], padding=1)), 1)
    cot = rnd(*ref.shape, seed=7)
    (ref * cot).sum().backward()
    g = [nhwc(x).to(dev), wu.to(dev), bu.to(dev), nhwc(s).to(dev), ws.to(dev), bs.to(dev)]
    g = [t.requires_grad_(True) for t in g]
    out = ops.UpCatFn.apply(*g, size)
    (out * nhwc(cot).to(dev)).sum().backward()
    assert rel_err(nchw(out), ref) < TOL
    for i, (a, r) in enumerate(zip(g, leaves)):
        ga = nchw(a.grad) if a.grad.dim() == 4 and i in (0, 3) else a.grad
        assert rel_err(ga, r.grad) < TOL_G, i


@pytest.mark.parametrize('C,training,with_res', [(16, True, False), (16, True, True), (24, True, False), (8, True, False),
                                                 (96, True, False), (128, True, True), (48, False, False), (32, False, True)])
def test_bn_lrelu(dev, C, training, with_res):
    from reconvat_amd import ops
    B, H, W = 2, 7, 13
    z = rnd(B, C, H, W, seed=1) * 2 + 0.3
    gamma, beta = rnd(C, seed=2) * 0.2 + 1, rnd(C, seed=3) * 0.1
    rm, rv = rnd(C, seed=4) * 0.1, rnd(C, seed=5).abs() + 0.5
    res = rnd(B, C, H, W, seed=6) if with_res else None
    zr, gr, br = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if with_res else None
    rmr, rvr = rm.clone(), rv.clone()
    yr = F.leaky_relu(F.batch_norm(zr, rmr, rvr, gr, br, training, 0.1, 1e-5))
    if with_res:
        yr = yr + rr
    cot = rnd(*yr.shape, seed=7)
    (yr * cot).sum().backward()
    zg = nhwc(z).to(dev).requires_grad_(True)
    gg, bg = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    rg = nhwc(res).to(dev).requires_grad_(True) if with_res else None
    rmg, rvg, nbt = rm.to(dev), rv.to(dev), torch.zeros((), dtype=torch.long, device=dev)
    yg = ops.BnActFn.apply(zg, gg, bg, rmg, rvg, nbt, rg, training, 0.01)
    (yg * nhwc(cot).to(dev)).sum().backward()
    assert rel_err(nchw(yg), yr) < TOL
    assert rel_err(nchw(zg.grad), zr.grad) < TOL_G
    assert rel_err(gg.grad, gr.grad) < TOL_G
    assert rel_err(bg.grad, br.grad) < TOL_G
    if with_res:
        assert rel_err(nchw(rg.grad), rr.grad) < TOL_G
    assert rel_err(rmg, rmr) < TOL and rel_err(rvg, rvr) < TOL
    assert int(nbt.item()) == (1 if training else 0)


@pytest.mark.autotune
@pytest.mark.parametrize('cin,cout,H,W', [(16, 16, 40, 229), (64, 32, 20, 57)])
def test_conv_autotuner(dev, cin, cout, H, W):
    """The tuner times every legal tile of both 3x3 kernels and caches a winner; whatever it picks must agree with the
    library default to fp32 rounding, with and without the fused BatchNorm statistics."""
    from reconvat_amd import ops
    x = nhwc(rnd(2, cin, H, W, seed=1)).to(dev)
    w, b = rnd(cout, cin, 3, 3, seed=2, scale=0.2).to(dev), rnd(cout, seed=3).to(dev)
    assert ops.AUTOTUNE
    stats = torch.zeros(ops.bn_ws_doubles(cout), dtype=torch.float64, device=dev)
    y_tuned = ops.ConvFn.apply(x, w, b, 'c3', None)
    y_tuned2 = ops.ConvFn.apply(x, w, b, 'c3', None, stats)
    assert any(k[:6] == (0, 2, H, W, cin, cout) for k in ops._algo_cache)
    ops.AUTOTUNE = False
    y_def = ops.ConvFn.apply(x, w, b, 'c3', None)
    assert rel_err(y_tuned, y_def) < 1e-5 and rel_err(y_tuned2, y_def) < 1e-5
    zd = y_tuned2.double().reshape(-1, cout)
    assert rel_err(stats.view(-1, 2 * cout).sum(0), torch.cat([zd.sum(0), (zd * zd).sum(0)])) < 1e-6


@pytest.mark.autotune
def test_online_tuner_offers_the_candidate_lists(dev, monkeypatch):
    """What the on-line tuner hands the library is tuning.conv_candidates / wgrad_candidates, in order; it keeps a candidate the library accepted,
    and the second launch of a shape tunes nothing.  (The smallest 3x3 shape that has every candidate family; no timing is asserted.)"""
    from reconvat_amd import _lib, ops, tuning
    lib = _lib.load()
    for name in ('_algo_cache', '_wgrad_tuned', '_wgrad_plans', '_wgrad_owner'):
        monkeypatch.setattr(tuning, name, type(getattr(tuning, name))())
    H, W, C = 16, 14, 16
    x, dy = nhwc(rnd(1, C, H, W, seed=1)).to(dev), nhwc(rnd(1, C, H, W, seed=4)).to(dev)
    w, b = rnd(C, C, 3, 3, seed=2, scale=0.2).to(dev), rnd(C, seed=3).to(dev)
    out = torch.empty_like(x)
    seen, conv_fwd, set_plan, wgrad = [], lib.rv_conv_fwd, lib.rv_conv_wgrad_set_plan, lib.rv_conv_wgrad

    def record(fn, what):
        def wrapped(*args):
            rc = fn(*args)
            seen.append((what(args), rc))
            return rc
        return wrapped

    def in_order(items):
        return list(dict.fromkeys(items))
    monkeypatch.setattr(lib, 'rv_conv_fwd', record(conv_fwd, lambda a: a[15]))
    ops.conv_forward_into('c3', x, w, b, out)
    cands = tuning.conv_candidates(0, H, W, C, C)
    assert {tuning.decode(c)[0] for c in cands} == {0, *tuning.FAMILIES} - {5, 14}
    assert in_order(a for a, _ in seen) == cands
    (key, chosen), = tuning._algo_cache.items()
    assert key[:6] == (0, 1, H, W, C, C) and (chosen, 0) in seen
    del seen[:]
    ops.conv_forward_into('c3', x, w, b, out)
    assert seen == [(chosen, 0)]                                         # cache hit: the launch itself, nothing else
    monkeypatch.setattr(lib, 'rv_conv_fwd', conv_fwd)

    del seen[:]
    monkeypatch.setattr(lib, 'rv_conv_wgrad_set_plan', record(set_plan, lambda a: tuple(a[5:7])))
    monkeypatch.setattr(lib, 'rv_conv_wgrad', record(wgrad, lambda a: 'launch'))
    try:
        ops.conv_wgrad('c3', x, dy, w)
        plans_seen = [(p, rc) for p, rc in seen if p != 'launch']
        assert in_order(p for p, _ in plans_seen) == tuning.wgrad_candidates(9, H) and len(tuning.wgrad_candidates(9, H)) == 9
        chosen = tuning._wgrad_plans[(9, 1, H, W, C, C)]
        assert seen[-2:] == [(chosen, 0), ('launch', 0)]                 # the winner is pinned, then the launch itself
        tried = seen[:-2]
        assert chosen in {p for (p, rc), nxt in zip(tried, tried[1:]) if p != 'launch' and rc == 0 and nxt == ('launch', 0)}
        del seen[:]
        ops.conv_wgrad('c3', x, dy, w)
        assert seen == [('launch', 0)]                                   # tuned: no plan is offered again
    finally:
        set_plan(9, 1, H, C, C, 0, 0)                                     # back to the library default partition
    torch.cuda.synchronize()


@pytest.mark.parametrize('cin,cout,H,W,algo', [(16, 16, 21, 37, 0), (32, 24, 9, 57, 0x221), (64, 128, 12, 28, 0x321), (16, 8, 10, 19, 0),
                                               (32, 32, 8, 30, 1), (1, 16, 9, 31, 0), (1, 16, 35, 150, 0), (1, 8, 19, 140, 0), (48, 24, 7, 114, 0x412),
                                               (32, 24, 11, 114, 0x723), (64, 128, 23, 57, 0x713), (8, 16, 12, 229, 0x716), (48, 32, 9, 57, 0x725)])
def test_conv_fused_bn_statistics(dev, cin, cout, H, W, algo, monkeypatch):
    """rv_conv_fwd(bn_sums=...) leaves sum / sum-of-squares of its output (fused epilogue of the persistent kernel,
    statistics pass behind the others), and BatchNorm on those sums equals BatchNorm computing its own."""
    from reconvat_amd import ops
    B = 3
    x = nhwc(rnd(B, cin, H, W, seed=1)).to(dev)
    w, b = rnd(cout, cin, 3, 3, seed=2, scale=0.2).to(dev), rnd(cout, seed=3).to(dev)
    if algo:
        monkeypatch.setenv('RV_FORCE_ALGO', hex(algo))
    stats = torch.zeros(ops.bn_ws_doubles(cout), dtype=torch.float64, device=dev)
    z = ops.ConvFn.apply(x, w, b, 'c3', None, stats)
    z0 = ops.ConvFn.apply(x, w, b, 'c3', None)
    assert torch.equal(z, z0)
    zd = z.double().reshape(-1, cout)
    want = torch.cat([zd.sum(0), (zd * zd).sum(0)])
    assert rel_err(stats.view(-1, 2 * cout).sum(0), want) < 1e-6
    gamma, beta = (rnd(cout, seed=4) * 0.2 + 1).to(dev), (rnd(cout, seed=5) * 0.1).to(dev)
    outs = []
    for st in (stats, None):
        rm, rv, nbt = torch.zeros(cout, device=dev), torch.ones(cout, device=dev), torch.zeros((), dtype=torch.long, device=dev)
        outs.append((ops.BnActFn.apply(z, gamma, beta, rm, rv, nbt, None, True, 0.01, st), rm, rv))
    assert rel_err(outs[0][0], outs[1][0]) < 1e-5
    assert rel_err(outs[0][1], outs[1][1]) < 1e-5 and rel_err(outs[0][2], outs[1][2]) < 1e-5


@pytest.mark.parametrize('cin,cout,H,W,algo', [(8, 8, 12, 229, 0x716), (32, 32, 23, 114, 0x723), (64, 64, 31, 57, 0x713), (24, 24, 11, 114, 0x715),
                                               (128, 128, 40, 28, 0x723), (96, 48, 21, 57, 0x733), (24, 40, 7, 114, 0x716), (32, 16, 3, 17, 0x713),
                                               (64, 32, 20, 57, 0x422), (32, 32, 9, 114, 0x324), (16, 16, 6, 229, 0x218)])
def test_conv3x3_forced_tile_vs_torch(dev, cin, cout, H, W, algo, monkeypatch):
    """Every wave count of the persistent 3x3 kernel (4 / 8 / 16 waves and the 12-wave family with 3 / 5 / 6 tiles per wave),
    forced per tile: forward and both gradients against torch's fp32 convolution; repeated launches bit-identical."""
    from reconvat_amd import ops
    monkeypatch.setenv('RV_FORCE_ALGO', hex(algo))
    B = 3
    x, w, b = rnd(B, cin, H, W, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.2), rnd(cout, seed=3)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yr = F.conv2d(*leaves, padding=1)
    cot = rnd(*yr.shape, seed=4)
    (yr * cot).sum().backward()
    g = [nhwc(x).to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)]
    yg = ops.ConvFn.apply(g[0], g[1], g[2], 'c3', None)
    (yg * nhwc(cot).to(dev)).sum().backward()
    assert rel_err(nchw(yg), yr) < TOL
    assert rel_err(nchw(g[0].grad), leaves[0].grad) < TOL_G
    assert rel_err(g[1].grad, leaves[1].grad) < TOL_G and rel_err(g[2].grad, leaves[2].grad) < TOL_G
    with torch.no_grad():
        for _ in range(5):
            assert torch.equal(ops.ConvFn.apply(g[0], g[1], g[2], 'c3', None), yg)


WINO_CASES = [(16, 16, 12, 229, 0x611), (32, 32, 22, 114, 0x611), (64, 64, 31, 57, 0x611), (16, 32, 9, 114, 0x611), (128, 128, 40, 28, 0x611),
              (96, 48, 21, 57, 0x611), (48, 24, 10, 114, 0x611), (32, 16, 3, 17, 0x611), (64, 32, 20, 57, 0xa11), (16, 16, 6, 57, 0xa11),
              (32, 32, 24, 114, 0x4611), (64, 64, 16, 28, 0x2611), (16, 8, 8, 229, 0x611),
              (32, 32, 22, 114, 0xa21), (64, 64, 31, 57, 0xa21), (128, 128, 40, 28, 0x8a21), (96, 64, 21, 57, 0xa21), (16, 16, 12, 229, 0xa11), (48, 48, 9, 57, 0xa11),
              (64, 64, 31, 57, 0xac11), (16, 16, 12, 229, 0xc11), (128, 128, 40, 28, 0xc11), (32, 16, 9, 114, 0x4c11),
              # round 4: rows of exactly one / two 1 KiB pieces, weights too large to stay resident (double-buffered per chunk), resident at 4 chunks
              (128, 128, 10, 14, 0x611), (32, 32, 8, 30, 0x611), (192, 96, 20, 28, 0x611), (64, 48, 12, 57, 0xa11), (192, 64, 9, 28, 0xc11),
              # round 5: the software-pipelined kernel (conv_wino2.hip) -- 0x8NM / 0x9NM: 8 waves with the full / half-chunk patch, 0xBNM / 0xDNM: 4 waves;
              # one chunk, resident weights, the three-slot weight ring (> 3 chunks that do not fit), ragged last bands, forced rows per band
              (16, 16, 12, 229, 0x811), (32, 32, 22, 114, 0x811), (64, 64, 31, 57, 0x811), (16, 32, 9, 114, 0x811), (128, 128, 40, 28, 0x811),
              (96, 48, 21, 57, 0x811), (48, 24, 10, 114, 0x811), (32, 16, 3, 17, 0x811), (192, 96, 20, 28, 0x811), (16, 8, 8, 229, 0x811),
              (64, 32, 20, 57, 0x911), (16, 16, 6, 57, 0x911), (32, 32, 22, 114, 0x921), (64, 64, 31, 57, 0x921), (128, 128, 40, 28, 0x8921),
              (96, 64, 21, 57, 0x921), (192, 96, 20, 28, 0x921), (64, 64, 31, 57, 0x912), (16, 16, 12, 229, 0x912), (128, 128, 40, 28, 0x912),
              (32, 32, 24, 114, 0x4811), (64, 64, 16, 28, 0x2811), (128, 128, 10, 14, 0x811), (32, 32, 8, 30, 0x811),
              (64, 64, 31, 57, 0xb12), (16, 16, 12, 229, 0xb12), (96, 48, 21, 57, 0xb12), (64, 64, 31, 57, 0xb21), (128, 128, 40, 28, 0xb21), (192, 96, 20, 28, 0xb21),
              # ... and its 12-wave form (0xDNM: three waves per SIMD, half-chunk patch)
              (64, 64, 31, 57, 0xad11), (16, 16, 12, 229, 0xd11), (128, 128, 40, 28, 0xd11), (32, 16, 9, 114, 0x4d11), (192, 64, 9, 28, 0xd11), (48, 32, 20, 57, 0xd11),
              # round 6: the half-CU experiment family 0xE (conv3x3_wino_k with four waves, <= 78 KiB of LDS, <= 256 registers, 512 workgroup slots;
              # never in the shipped table -- tools/pair_probe.py set4, profiles/r06_half_cu_pairs.txt)
              (128, 128, 40, 28, 0xe11), (64, 64, 31, 57, 0xe11), (64, 128, 20, 28, 0xe11), (192, 96, 20, 28, 0xe11), (32, 32, 8, 30, 0xe11)]


@pytest.mark.parametrize('cin,cout,H,W,algo', WINO_CASES)
def test_conv3x3_winograd_vs_torch(dev, cin, cout, H, W, algo, monkeypatch):
    """Winograd F(2x2,3x3) form of the persistent 3x3 kernel (families 0x6NM / 0xANM / 0xCNM, forced): forward and both gradients (the input
    gradient runs the same kernel on the flipped / transposed weights) against torch's fp32 convolution, odd and even widths and
    heights, ragged last bands, fused statistics; repeated launches bit-identical."""
    from reconvat_amd import ops
    monkeypatch.setenv('RV_FORCE_ALGO', hex(algo))
    B = 3
    x, w, b = rnd(B, cin, H, W, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=0.2), rnd(cout, seed=3)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yr = F.conv2d(*leaves, padding=1)
    cot = rnd(*yr.shape, seed=4)
    (yr * cot).sum().backward()
    g = [nhwc(x).to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)]
    stats = torch.zeros(ops.bn_ws_doubles(cout), dtype=torch.float64, device=dev)
    yg = ops.ConvFn.apply(g[0], g[1], g[2], 'c3', None, stats)
    if cout % 16:
        monkeypatch.delenv('RV_FORCE_ALGO')              # (the input gradient of a narrower output has 8-channel chunks: direct form)
    (yg * nhwc(cot).to(dev)).sum().backward()
    assert rel_err(nchw(yg), yr) < 2 * TOL
    zd = yg.detach().double().reshape(-1, cout)
    assert rel_err(stats.view(-1, 2 * cout).sum(0), torch.cat([zd.sum(0), (zd * zd).sum(0)])) < 1e-6
    assert rel_err(nchw(g[0].grad), leaves[0].grad) < 2 * TOL_G
    assert rel_err(g[1].grad, leaves[1].grad) < TOL_G and rel_err(g[2].grad, leaves[2].grad) < TOL_G
    if cout % 16 == 0:
        with torch.no_grad():
            for _ in range(5):
                assert torch.equal(ops.ConvFn.apply(g[0], g[1], g[2], 'c3', None), yg)


@pytest.mark.parametrize('cin,cout,H,W,algo', [(32, 32, 22, 114, 0x611), (64, 32, 13, 57, 0xa21), (16, 16, 10, 229, 0xc11), (48, 16, 9, 57, 0xa11),
                                               (32, 32, 22, 114, 0x811), (64, 32, 13, 57, 0x921), (16, 16, 10, 229, 0x911), (48, 16, 9, 57, 0xb12)])
def test_conv3x3_winograd_accumulate_and_colsum(dev, cin, cout, H, W, algo, monkeypatch):
    """The Winograd form behind the other two epilogue options of the persistent kernel: ``accumulate`` (a GradShare consumer adds its
    input gradient into the shared buffer) and the plain per-channel sums of what it stores (ColsumLink) -- against the direct form."""
    from reconvat_amd import ops
    B = 3
    dy = nhwc(rnd(B, cout, H, W, seed=1)).to(dev)
    w = rnd(cout, cin, 3, 3, seed=2, scale=0.2).to(dev)
    base = nhwc(rnd(B, cin, H, W, seed=3)).to(dev)
    outs = []
    for forced in (algo, 0x111):
        monkeypatch.setenv('RV_FORCE_ALGO', hex(forced))
        ops.invalidate_weight_cache()
        dx = base.clone()
        ops.conv_dgrad_into('c3', dy, w, dx, accumulate=True)
        sums = torch.zeros(ops.bn_ws_doubles(cin), dtype=torch.float64, device=dev)
        dx2 = torch.empty_like(base)
        ops.conv_dgrad_into('c3', dy, w, dx2, sum_ws=sums)
        outs.append((dx, dx2, sums.view(-1, 2 * cin).sum(0)[:cin]))
    assert rel_err(outs[0][0], outs[1][0]) < 4e-5 and rel_err(outs[0][1], outs[1][1]) < 4e-5
    assert rel_err(outs[0][0] - base, outs[0][1]) < 4e-5
    assert rel_err(outs[0][2], outs[0][1].double().reshape(-1, cin).sum(0)) < 1e-6
    assert rel_err(outs[0][2], outs[1][2]) < 1e-5


@pytest.mark.parametrize('algo', ['0xc11', '0xd11', '0x921'])
def test_winograd_12_wave_tile_refuses_the_fused_bn_backward(dev, monkeypatch, algo):
    """Three waves per SIMD leave 168 registers: the fused BatchNorm-backward epilogue of the Winograd kernels (0xc11, and the pipelined
    kernel's 0xd11) does not fit them without scratch, and neither does it fit the pipelined kernel's 8-wave NT = 2 half-chunk tile
    (0x921), so those combinations are refused (the tuner never offers them) instead of silently spilling."""
    from reconvat_amd import ops, _lib
    monkeypatch.setenv('RV_FORCE_ALGO', algo)
    x = torch.rand(2, 10, 57, 32, device=dev)
    w = torch.rand(32, 32, 3, 3, device=dev)
    link = ops.BnLink()
    z = torch.rand(2, 10, 57, 32, device=dev)
    link.z, link.coef, link.ws, link.slope = z, torch.rand(5 * 32, device=dev), torch.zeros(ops.bn_ws_doubles(32), dtype=torch.float64, device=dev), 0.01
    with pytest.raises(RuntimeError, match='does not fit'):
        ops.conv_dgrad_into('c3', x, w, torch.empty_like(x), bn_link=link)
    ops.conv_dgrad_into('c3', x, w, torch.empty_like(x))           # ... the plain launch of the same tile is fine
    torch.cuda.synchronize()


@pytest.mark.parametrize('c1,c2,H,W,algo', [(16, 16, 12, 37, 0), (24, 16, 9, 57, 0x211), (64, 32, 8, 28, 0x321), (8, 2, 6, 19, 0), (8, 2, 37, 300, 0), (32, 32, 8, 30, 1),
                                            (24, 16, 11, 114, 0x713), (64, 24, 9, 57, 0x726), (32, 32, 11, 114, 0x611), (16, 16, 9, 57, 0x611), (48, 32, 8, 28, 0xa11), (64, 64, 12, 57, 0xa21), (48, 48, 14, 229, 0x611), (96, 32, 9, 114, 0xa11),
                                            (32, 32, 11, 114, 0x811), (16, 16, 9, 57, 0x811), (48, 32, 8, 28, 0x911), (16, 16, 14, 229, 0x811), (64, 64, 12, 57, 0xb12)])
def test_conv_dgrad_fused_bn_backward_reduction(dev, c1, c2, H, W, algo, monkeypatch):
    """conv2(lrelu(bn(z))): with a BnLink the input-gradient kernel of conv2 also produces the BatchNorm's backward
    reduction (epilogue of the persistent kernel, reduction pass behind the others); gradients must not change."""
    from reconvat_amd import ops
    B = 3
    if algo:
        monkeypatch.setenv('RV_FORCE_ALGO', hex(algo))
    z0 = nhwc(rnd(B, c1, H, W, seed=1) * 2 + 0.3).to(dev)
    g0, b0 = (rnd(c1, seed=2) * 0.2 + 1).to(dev), (rnd(c1, seed=3) * 0.1).to(dev)
    w0, wb0 = rnd(c2, c1, 3, 3, seed=4, scale=0.2).to(dev), rnd(c2, seed=5).to(dev)
    cot = nhwc(rnd(B, c2, H, W, seed=6)).to(dev)
    grads = []
    for use_link in (True, False):
        z, g, b, w, wb = [t.clone().requires_grad_(True) for t in (z0, g0, b0, w0, wb0)]
        rm, rv, nbt = torch.zeros(c1, device=dev), torch.ones(c1, device=dev), torch.zeros((), dtype=torch.long, device=dev)
        link = ops.BnLink() if use_link else None
        y = ops.BnActFn.apply(z, g, b, rm, rv, nbt, None, True, 0.01, None, link)
        o = ops.ConvFn.apply(y, w, wb, 'c3', None, None, link)
        (o * cot).sum().backward()
        grads.append([t.grad.clone() for t in (z, g, b, w, wb)])
    for a, b_ in zip(*grads):
        assert rel_err(a, b_) < 2e-5


@pytest.mark.parametrize('kind,cin,cout,H,W', [('c3', 32, 32, 24, 57), ('c3', 48, 24, 17, 114), ('c1', 16, 32, 30, 28), ('down', 16, 16, 22, 38)])
def test_wgrad_partition_plans_agree(dev, kind, cin, cout, H, W):
    """rv_conv_wgrad_set_plan (the weight-gradient partition the autotuner pins per shape): every plan -- 4 or 8 waves per
    workgroup, 128 .. 1024 workgroups -- must give the torch weight / bias gradient to fp32 rounding, and the default again
    after the plan is cleared."""
    from reconvat_amd import ops, _lib
    lib = _lib.load()
    B = 3
    x = rnd(B, cin, H, W, seed=1)
    stride, ksz = (2, 2) if kind == 'down' else (1, 3 if kind == 'c3' else 1)
    w = rnd(cout, cin, ksz, ksz, seed=2, scale=0.2).requires_grad_(True)
    b = rnd(cout, seed=3).requires_grad_(True)
    y = F.conv2d(x, w, b, stride=stride, padding=1 if kind == 'c3' else 0)
    cot = rnd(*y.shape, seed=4)
    (y * cot).sum().backward()
    xg, dyg, wg = nhwc(x).to(dev), nhwc(cot).to(dev), w.detach().to(dev)
    taps = ksz * ksz
    ho, wo = y.shape[2], y.shape[3]
    try:
        for nw, wgs in ((0, 0), (4, 128), (4, 512), (8, 256), (8, 1024), (0, 0)):
            assert lib.rv_conv_wgrad_set_plan(taps, B, ho, cin, cout, nw, wgs) == 0
            dw, db = ops.conv_wgrad(kind, xg, dyg, wg)
            assert rel_err(dw, w.grad) < TOL_G, (nw, wgs)
            assert rel_err(db, b.grad) < TOL_G, (nw, wgs)
    finally:
        lib.rv_conv_wgrad_set_plan(taps, B, ho, cin, cout, 0, 0)
    assert lib.rv_conv_wgrad_set_plan(taps, B, ho, cin, cout, 3, 0) != 0          # waves must be 0 / 4 / 8


@pytest.mark.parametrize('M,K,N,act', [(130, 229, 88, 1), (257, 176, 768, 0), (64, 768, 88, 1), (200, 916, 229, 1), (96, 88, 916, 0)])
def test_linear(dev, M, K, N, act):
    from reconvat_amd import ops
    x, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yr = F.linear(*leaves)
    if act:
        yr = torch.sigmoid(yr)
    cot = rnd(M, N, seed=4)
    (yr * cot).sum().backward()
    g = [t.to(dev).requires_grad_(True) for t in (x, w, b)]
    yg = ops.LinearFn.apply(g[0], g[1], g[2], act)
    (yg * cot.to(dev)).sum().backward()
    assert rel_err(yg, yr) < TOL
    for a, r in zip(g, leaves):
        assert rel_err(a.grad, r.grad) < TOL_G


def test_onset_heads(dev):
    from reconvat_amd import ops
    B, T = 2, 37
    y = rnd(B, 2, T, 229, seed=1)
    wo, bo, wf, bf = rnd(88, 229, seed=2, scale=0.1), rnd(88, seed=3), rnd(88, 229, seed=4, scale=0.1), rnd(88, seed=5)
    leaves = [t.clone().requires_grad_(True) for t in (y, wo, bo, wf, bf)]
    onset = torch.sigmoid(F.linear(leaves[0][:, 0], leaves[1], leaves[2]))
    feat = F.linear(leaves[0][:, 1], leaves[3], leaves[4])
    cat = torch.cat((onset, feat), -1)
    c1, c2 = rnd(B, T, 176, seed=6), rnd(B, T, 88, seed=7)
    ((cat * c1).sum() + (onset * c2).sum()).backward()
    g = [nhwc(y).to(dev)] + [t.to(dev) for t in (wo, bo, wf, bf)]
    g = [t.requires_grad_(True) for t in g]
    catg, onsetg = ops.OnsetHeadsFn.apply(*g)
    ((catg.view(B, T, 176) * c1.to(dev)).sum() + (onsetg.view(B, T, 88) * c2.to(dev)).sum()).backward()
    assert rel_err(catg.view(B, T, 176), cat) < TOL and rel_err(onsetg.view(B, T, 88), onset) < TOL
    assert rel_err(nchw(g[0].grad), leaves[0].grad) < TOL_G
    for a, r in zip(g[1:], leaves[1:]):
        assert rel_err(a.grad, r.grad) < TOL_G


@pytest.mark.parametrize('fin,fout,groups,L', [(176, 768, 6, 50), (88, 916, 4, 33), (229, 916, 4, 16)])
def test_local_attention(dev, fin, fout, groups, L):
    from oracle import model as om
    from reconvat_amd import ops
    B = 2
    p = {'a.rel': rnd(1, fout, 31, seed=1, scale=0.5)}
    for i, w in enumerate(('W_q', 'W_k', 'W_v')):
        p[f'a.{w}.weight'] = rnd(fout, fin, seed=2 + i, scale=float(np.sqrt(3.0 / fin)))
    x = rnd(B, L, fin, seed=9)
    cot = rnd(B, L, fout, seed=10)
    po = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xo = x.clone().requires_grad_(True)
    oo, ao = om.local_attention(om.Net(po), xo, 'a', groups)
    (oo * cot).sum().backward()
    g = {k: v.to(dev).requires_grad_(True) for k, v in p.items()}
    xg = x.to(dev).requires_grad_(True)
    og, ag = ops.LocalAttnFn.apply(xg, g['a.W_q.weight'], g['a.W_k.weight'], g['a.W_v.weight'], g['a.rel'], groups)
    (og * cot.to(dev)).sum().backward()
    assert rel_err(og, oo) < TOL and rel_err(ag, ao) < TOL
    assert rel_err(xg.grad, xo.grad) < TOL_G
    for k in p:
        assert rel_err(g[k].grad, po[k].grad) < TOL_G, k


def test_attention_golden(dev):
    """Same op against the vectors the reference itself produced (tests/golden/attention.npz)."""
    import os
    from oracle import fixture as fx
    from reconvat_amd import ops
    gold = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'attention.npz'))
    for tag, fin, fout, groups in (('t176', 176, 768, 6), ('r88', 88, 916, 4), ('f229', 229, 916, 4)):
        rel = fx.hashed_normalish(tag + 'rel', (1, fout, 31), 0.5).to(dev).requires_grad_(True)
        ws = [fx.hashed(tag + w, (fout, fin), float(np.sqrt(3.0 / fin))).to(dev).requires_grad_(True) for w in ('W_q', 'W_k', 'W_v')]
        x = fx.hashed(tag + 'x', (2, 64, fin), 1.0).to(dev).requires_grad_(True)
        cot = fx.hashed(tag + 'cot', (2, 64, fout), 1.0).to(dev)
        o, a = ops.LocalAttnFn.apply(x, ws[0], ws[1], ws[2], rel, groups)
        (o * cot).sum().backward()
        assert rel_err(o, torch.from_numpy(gold[tag + '_out'])) < TOL
        assert rel_err(a, torch.from_numpy(gold[tag + '_att'])) < TOL
        assert rel_err(x.grad, torch.from_numpy(gold[tag + '_dx'])) < TOL_G
        assert rel_err(rel.grad, torch.from_numpy(gold[tag + '_drel'])) < TOL_G


def test_losses(dev):
    from reconvat_amd import ops
    p = torch.sigmoid(rnd(3, 70, 88, seed=1) * 4)
    p.view(-1)[:4] = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-8])     # exercises the -100 log clamp
    t_soft = torch.sigmoid(rnd(3, 70, 88, seed=2) * 3)
    t_hard = (rnd(3, 70, 88, seed=3) > 0.8).float()
    for t in (t_soft, t_hard):
        pr = p.clone().requires_grad_(True)
        lr = F.binary_cross_entropy(pr, t)
        (lr * 1.7).backward()
        pg = p.to(dev).requires_grad_(True)
        lg = ops.bce_mean(pg, t.to(dev))
        (lg * 1.7).backward()
        assert rel_err(lg, lr) < TOL and rel_err(pg.grad, pr.grad) < TOL_G
    a, b = rnd(2, 50, 229, seed=4), rnd(2, 50, 229, seed=5)
    ar = a.clone().requires_grad_(True)
    lr = F.mse_loss(ar, b)
    lr.backward()
    ag = a.to(dev).requires_grad_(True)
    lg = ops.mse_mean(ag, b.to(dev))
    lg.backward()
    assert rel_err(lg, lr) < TOL and rel_err(ag.grad, ar.grad) < TOL_G
    assert rel_err(ops.abs_mean(a.to(dev)), a.abs().mean()) < TOL
    assert rel_err(ops.l2_norm(a.to(dev)), a.norm()) < TOL


def test_vat_perturb(dev):
    from reconvat_amd import ops
    x = rnd(2, 1, 33, 229, seed=1) * 0.5 + 0.5
    x.view(-1)[:50] = 0.0
    x.view(-1)[50:100] = 1.0                               # clamp is active on these
    d = rnd(2, 1, 33, 229, seed=2)
    for xi in (1e-1, 1e-6):
        dr = d.clone().requires_grad_(True)
        xa = (x + xi * dr / torch.norm(dr, dim=-1, keepdim=True)).clamp(0, 1)
        cot = rnd(*x.shape, seed=3)
        (xa * cot).sum().backward()
        dg = d.to(dev).requires_grad_(True)
        xg = ops.VatPerturbFn.apply(x.to(dev), dg, xi)
        (xg * cot.to(dev)).sum().backward()
        assert rel_err(xg, xa) < 1e-6
        assert rel_err(dg.grad, dr.grad) < TOL_G
    g = rnd(2, 1, 33, 229, seed=4) * 1e-11
    dd = g * 1e10
    dn = dd / torch.norm(dd, dim=-1, keepdim=True)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    xa, r, dng = ops.vat_adversarial(x.to(dev), g.to(dev), 1e10, 2.0, flag)
    assert rel_err(r, 2.0 * dn) < 1e-5 and rel_err(dng, dn) < 1e-5
    assert rel_err(xa, (x + 2.0 * dn).clamp(0, 1)) < 1e-5
    assert int(flag.item()) == 0
    g[0, 0, 3] = 0.0                                        # 0/0 -> NaN row -> flag, like the reference's assert
    ops.vat_adversarial(x.to(dev), g.to(dev), 1e10, 2.0, flag)
    assert int(flag.item()) == 1


def test_frontend(dev):
    import os
    from oracle import fixture as fx, frontend as ofe
    from reconvat_amd.frontend import MelSpectrogram
    gold = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'frontend.npz'))
    m = MelSpectrogram().to(dev)
    audio = fx.fixture_audio(2, 65536)[:, :-1]
    mel = m(audio.to(dev))
    assert mel.shape == (2, 229, 128)
    assert rel_err(mel, torch.from_numpy(gold['mel'])) < 1e-4
    ln = m.lognorm(audio.to(dev))
    assert ln.shape == (2, 1, 128, 229)
    err = (ln.cpu() - torch.from_numpy(gold['lognorm'])).abs().max().item()
    assert err < 1e-4, err                                 # values span [0,1]; north-star tolerance 1e-3
    assert ln.min().item() == 0.0 and ln.max().item() == 1.0
    bufs = ofe.frontend_buffers()
    a2 = fx.fixture_audio(3, 40000, 'odd')[:, :-1]          # ragged length, 3 clips
    ref = ofe.frontend(a2, bufs)
    got = m.lognorm(a2.to(dev))
    assert got.shape == ref.shape
    assert (got.cpu() - ref).abs().max().item() < 1e-4


def test_adam(dev):
    from reconvat_amd.train import FlatAdam
    ps = [torch.nn.Parameter(rnd(7, 5, seed=1)), torch.nn.Parameter(rnd(33, seed=2)), torch.nn.Parameter(rnd(4, 3, 2, seed=3))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    gp = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ps]
    o_ref = torch.optim.Adam(ref, 1e-3)
    sch = torch.optim.lr_scheduler.StepLR(o_ref, step_size=3, gamma=0.5)
    o = FlatAdam(gp, lr=1e-3, step_size=3, gamma=0.5)
    for it in range(7):
        o.zero_grad()
        o_ref.zero_grad()
        for i, (a, r) in enumerate(zip(gp, ref)):
            if i == 1:
                continue                                     # a parameter that never receives a gradient
            g = rnd(*a.shape, seed=10 * it + i)
            r.grad = g.clone()
            a.grad.copy_(g.to(dev))
        o.step()
        o_ref.step()
        sch.step()
    for a, r in zip(gp, ref):
        assert rel_err(a, r) < 1e-5
    assert abs(o.current_lr() - o_ref.param_groups[0]['lr']) < 1e-12


@pytest.mark.parametrize('M,N,K,kw', [
    (5120, 2304, 176, {}),                                   # fused [k|q|v] projection, 128-row blocks
    (5120, 176, 2304, {'splitk': 2}),                        # its input gradient through the transposed weight copy
    (5120, 88, 768, {'act': 1, 'bias': True}),               # narrow N: 64-row blocks, sigmoid epilogue
    (5120, 229, 916, {'act': 1, 'bias': True}),              # K tail (916 = 28 x 32 + 20), N not a multiple of 4 -> scalar stores
    (333, 100, 88, {'bias': True, 'c2': True}),              # ragged M / N, second destination
    (200, 72, 40, {'accumulate': True}),                     # K of a single partial stage, C += 
    (64, 64, 4, {}),                                         # smallest legal problem
])
def test_gemm_k_contiguous_full_size(dev, M, N, K, kw):
    """rv_gemm with two K-contiguous, 16-byte aligned operands (the forward and -- through ops._lin_t -- input-gradient
    GEMMs of the step) at the step's shapes, against torch.matmul in fp64; and against the same product from an unaligned
    view (scalar-load path of the kernel)."""
    from reconvat_amd import ops
    a, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.2)
    bias = rnd(N, seed=3) if kw.get('bias') else None
    ref = a.double() @ b.double().t()
    if bias is not None:
        ref = ref + bias.double()
    if kw.get('act'):
        ref = torch.sigmoid(ref)
    c0 = rnd(M, N, seed=4)
    if kw.get('accumulate'):
        ref = ref + c0.double()
    ag, bg = a.to(dev), b.to(dev)
    c = c0.to(dev).clone() if kw.get('accumulate') else torch.full((M, N), float('nan'), device=dev)
    c2 = torch.full((N, M), float('nan'), device=dev) if kw.get('c2') else None
    ops.gemm(ag, bg.t(), c, bias.to(dev) if bias is not None else None, act=kw.get('act', 0), accumulate=bool(kw.get('accumulate')),
             splitk=kw.get('splitk', 1), c2=c2.t() if c2 is not None else None)
    assert rel_err(c, ref.float()) < 2e-5
    if c2 is not None:
        assert rel_err(c2.t(), ref.float()) < 2e-5
    # the same product from an operand that is not 16-byte aligned
    if not kw.get('accumulate') and not kw.get('splitk'):
        pad = torch.zeros(M, K + 1, device=dev)
        pad[:, 1:] = ag
        c3 = torch.empty((M, N), device=dev)
        ops.gemm(pad[:, 1:], bg.t(), c3, bias.to(dev) if bias is not None else None, act=kw.get('act', 0))
        assert rel_err(c3, c) < 2e-5


def test_grouped_deferred_gemms_vs_torch(dev):
    """ops.deferred_param_gemms: accumulating GEMMs of different shapes (one batched, one with the row-sum rider, split-K and not)
    registered and run as ONE grouped launch (rv_gemm_table_run) -- each destination must equal its start value + A @ B."""
    from reconvat_amd import ops
    torch.manual_seed(0)
    cases = [(88, 229, 1280, 1, 4), (88, 768, 1280, 1, 8), (300, 176, 640, 1, 1), (128, 31, 1280, 3, 4)]
    items = []
    for m, n, k, batch, sk in cases:
        at = torch.randn(batch, k, m, device=dev)            # A = at^T (M-fast, like dY^T)
        b = torch.randn(batch, k, n, device=dev)
        c = torch.randn(batch, m, n, device=dev)
        items.append((at, b, c, c.clone(), sk, batch))
    rs = torch.randn(88, device=dev)
    rs0 = rs.clone()
    with ops.deferred_param_gemms() as pend:
        for i, (at, b, c, c0, sk, batch) in enumerate(items):
            ops.gemm(at[0].t(), b[0], c[0], accumulate=True, splitk=sk, deterministic=False, batch=batch,
                     bstrides=(at.stride(0), b.stride(0), c.stride(0)), a_rowsum=rs if i == 0 else None, defer_ok=True)
        torch.cuda.synchronize()
        assert all(torch.equal(c, c0) for _, _, c, c0, _, _ in items), 'nothing may run before flush()'
        # without the explicit opt-in (a destination autograd may read before the flush) the GEMM runs at once, context or not
        tmp, tmp0 = items[0][2][0].clone(), items[0][2][0].clone()
        ops.gemm(items[0][0][0].t(), items[0][1][0], tmp, accumulate=True, splitk=4, deterministic=False)
        torch.cuda.synchronize()
        assert not torch.equal(tmp, tmp0)
        assert sum(t.n for t in pend.tables.values()) == len(items)
        pend.flush()
    torch.cuda.synchronize()
    for at, b, c, c0, sk, batch in items:
        want = c0.double() + torch.einsum('zkm,zkn->zmn', at.double(), b.double())
        assert rel_err(c, want.float()) < 1e-5
    assert rel_err(rs, (rs0.double() + items[0][0][0].double().sum(0)).float()) < 1e-5


@pytest.mark.parametrize('cin,cout,h,w,algo', [(16, 16, 40, 57, 0), (32, 64, 20, 28, 0x713), (64, 32, 24, 57, 0x422), (128, 128, 10, 14, 0x321),
                                               (48, 96, 16, 57, 0x212), (192, 96, 10, 28, 0)])
def test_conv3x3_bf16_operands_vs_torch(dev, cin, cout, h, w, algo):
    """The opt-in bf16-operand variant of the persistent 3x3 kernel (rv_conv_fwd algo bit 20): equals a plain fp32 convolution of
    the bf16-ROUNDED operands (products of bf16 numbers are exact in fp32; accumulation is fp32 in both), and differs from the
    fp32 kernel by about 2^-9 relative -- i.e. the bit really selects the bf16 matrix instructions."""
    import torch.nn.functional as F
    from reconvat_amd import ops
    B = 3
    x = rnd(B, h, w, cin, seed=1).to(dev)
    wt = (rnd(cout, cin, 3, 3, seed=2) * (1.0 / (9 * cin) ** 0.5)).to(dev)
    bias = rnd(cout, seed=3).to(dev)
    rb = lambda t: t.to(torch.bfloat16).to(torch.float32)
    ref_bf = F.conv2d(rb(x).cpu().permute(0, 3, 1, 2), rb(wt).cpu(), bias.cpu(), padding=1).permute(0, 2, 3, 1)
    ref_32 = F.conv2d(x.cpu().permute(0, 3, 1, 2), wt.cpu(), bias.cpu(), padding=1).permute(0, 2, 3, 1)
    out = torch.empty(B, h, w, cout, device=dev)
    pack = ops._pack('c3', wt, 'fwd')
    args = (0, x.data_ptr(), cin, B, h, w, cin, out.data_ptr(), cout, h, w, cout, pack.data_ptr(), bias.data_ptr(), 0)
    from reconvat_amd import _lib
    lib = _lib.load()
    rc = lib.rv_conv_fwd(*args, algo | ops.ALGO_BF16, None, None, 0, None, 0.0, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        pytest.skip('tile does not fit this shape')
    torch.cuda.synchronize()
    assert rel_err(out, ref_bf) < 2e-5
    d32 = rel_err(out, ref_32)
    assert 2e-4 < d32 < 2e-2, d32


@pytest.mark.parametrize('algo', [0x811, 0x911, 0xb12, 0x611, 0xa11])
def test_bf16_launch_of_a_winograd_plan_runs_a_bf16_kernel(dev, algo, monkeypatch):
    """a shape whose plan entry is an fp32 Winograd tile (conv3x3_wino_k 0x6 / 0xA / 0xC, conv3x3_wino2_k 0x8 / 0x9 / 0xB / 0xD)
    has no bf16 form; a bf16 launch through the host wrapper must fall back to the library-default direct tile WITH the bf16 bit --
    not keep the Winograd algo, whose launcher strips the bit and runs fp32 (a silent no-op that bench.py would grade as bf16)."""
    from reconvat_amd import ops
    monkeypatch.setenv('RV_FORCE_ALGO', hex(algo))
    assert (algo >> 8) & 15 in ops.WINOGRAD_FAMILIES
    B, h, w, cin, cout = 2, 24, 57, 64, 64
    x = rnd(B, h, w, cin, seed=1).to(dev)
    wt = (rnd(cout, cin, 3, 3, seed=2) * (1.0 / (9 * cin) ** 0.5)).to(dev)
    bias = rnd(cout, seed=3).to(dev)
    rb = lambda t: t.to(torch.bfloat16).to(torch.float32)
    ref_bf = F.conv2d(rb(x).cpu().permute(0, 3, 1, 2), rb(wt).cpu(), bias.cpu(), padding=1).permute(0, 2, 3, 1)
    ref_32 = F.conv2d(x.cpu().permute(0, 3, 1, 2), wt.cpu(), bias.cpu(), padding=1).permute(0, 2, 3, 1)
    seen = []
    from reconvat_amd import _lib

    def hook(name, args, fn):
        if name == 'rv_conv_fwd':
            seen.append(args[15])
        return fn(*args)
    monkeypatch.setattr(_lib, 'HOOK', [hook])
    out = torch.empty(B, h, w, cout, device=dev)
    ops.conv_forward_into('c3', x, wt, bias, out, bf16=True)
    out32 = torch.empty(B, h, w, cout, device=dev)
    ops.conv_forward_into('c3', x, wt, bias, out32, bf16=False)
    torch.cuda.synchronize()
    assert len(seen) == 2 and seen[0] & ops.ALGO_BF16 and (seen[0] >> 8) & 15 not in ops.WINOGRAD_FAMILIES, [hex(a) for a in seen]
    assert seen[1] == algo                                     # the fp32 launch keeps its Winograd tile
    assert rel_err(out, ref_bf) < 2e-5                         # bf16-rounded operands, fp32 accumulate: the bf16 matrix instructions ran
    assert 2e-4 < rel_err(out, ref_32) < 2e-2
    assert rel_err(out32, ref_32) < 1e-5


@pytest.mark.parametrize('kind,cin,cout,h,w', [('c3', 16, 16, 24, 229), ('c3', 32, 32, 20, 114), ('t3', 96, 48, 12, 57), ('c3', 64, 128, 10, 28),
                                              ('t3', 192, 96, 10, 28), ('c3', 48, 24, 9, 114), ('c3', 16, 32, 7, 33)])
def test_wgrad3x3_bf16_operands_vs_torch(dev, kind, cin, cout, h, w):
    """The opt-in bf16-operand variant of the 3x3 weight-gradient kernel (rv_conv_wgrad mode bit 8): equals torch's weight gradient
    of the bf16-ROUNDED operands (fp32 accumulation in both), bias gradient exact fp32, and sits ~2^-9 away from the fp32 kernel."""
    from reconvat_amd import ops
    B = 3
    x, dy = rnd(B, h, w, cin, seed=5), rnd(B, h, w, cout, seed=6)
    rb = lambda t: t.to(torch.bfloat16).to(torch.float32)

    def ref(xx, dd):
        wt = torch.zeros((cout, cin, 3, 3) if kind == 'c3' else (cin, cout, 3, 3), requires_grad=True)
        y = F.conv2d(nchw(xx), wt, None, padding=1) if kind == 'c3' else F.conv_transpose2d(nchw(xx), wt, None, padding=1)
        (y * nchw(dd)).sum().backward()
        return wt.grad
    want_bf, want_32 = ref(rb(x), rb(dy)), ref(x, dy)
    wdev = torch.zeros_like(want_32).to(dev)
    dw, db = ops.conv_wgrad(kind, x.to(dev), dy.to(dev), wdev, True, bf16=True)
    torch.cuda.synchronize()
    assert rel_err(dw, want_bf) < 5e-5
    assert rel_err(db, dy.reshape(-1, cout).double().sum(0).float()) < 1e-5
    assert 1e-4 < rel_err(dw, want_32) < 3e-2


@pytest.mark.parametrize('kind,cin,cout,H,W,algo', [('down', 128, 128, 10, 14, 0x521), ('down', 64, 64, 12, 28, 0x512), ('down', 192, 64, 9, 21, 0x511),
                                                    ('c1', 64, 128, 7, 28, 0x522), ('up', 128, 128, 5, 7, 0x541), ('up', 64, 64, 6, 14, 0x514)])
def test_direct_conv_in_workgroup_splitk_vs_torch(dev, kind, cin, cout, H, W, algo, monkeypatch):
    """Family 0x5NM of the direct kernel (the four waves of a workgroup split the K loop and fold through LDS): forward and both
    gradients of the 1x1 / 2x2 conv kinds against torch (the backward uses the same family for the transposed role)."""
    from reconvat_amd import ops
    monkeypatch.setenv('RV_FORCE_ALGO', hex(algo))
    monkeypatch.setenv('RV_FORCE_ALGO_ALL', '1')
    B = 3
    x = rnd(B, cin, H, W, seed=1)
    if kind == 'down':
        w, ref = rnd(cout, cin, 2, 2, seed=2, scale=0.2), lambda x_, w_, b_: F.conv2d(x_, w_, b_, stride=2)
    elif kind == 'c1':
        w, ref = rnd(cout, cin, 1, 1, seed=2, scale=0.2), lambda x_, w_, b_: F.conv2d(x_, w_, b_)
    else:
        w, ref = rnd(cin, cout, 2, 2, seed=2, scale=0.2), lambda x_, w_, b_: F.conv_transpose2d(x_, w_, b_, stride=2, output_padding=(0, 1))
    b = rnd(cout, seed=3)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yr = ref(*leaves)
    cot = rnd(*yr.shape, seed=4)
    (yr * cot).sum().backward()
    g = [nhwc(x).to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)]
    size = (yr.shape[2], yr.shape[3]) if kind == 'up' else None
    yg = ops.ConvFn.apply(g[0], g[1], g[2], kind, size)
    (yg * nhwc(cot).to(dev)).sum().backward()
    assert rel_err(nchw(yg), yr) < TOL
    assert rel_err(nchw(g[0].grad), leaves[0].grad) < TOL_G
    assert rel_err(g[1].grad, leaves[1].grad) < TOL_G and rel_err(g[2].grad, leaves[2].grad) < TOL_G


WGRAD_WINO_CASES = [('c3', 32, 32, 12, 57), ('c3', 64, 64, 8, 28), ('t3', 96, 48, 10, 57), ('c3', 16, 16, 6, 229), ('c3', 48, 24, 8, 114),
                    ('t3', 192, 96, 4, 28), ('c3', 16, 32, 4, 114), ('c3', 128, 128, 6, 14), ('c3', 24, 16, 4, 37), ('t3', 16, 8, 6, 229)]


@pytest.mark.parametrize('kind,cin,cout,H,W', WGRAD_WINO_CASES)
def test_wgrad_winograd_form_vs_torch(dev, kind, cin, cout, H, W):
    """The Winograd F(3x3, 2x2) weight-gradient kernel (plan code nw = 24): dW and db of Conv2d / ConvTranspose2d 3x3 against torch
    autograd -- odd and even widths, channel counts that pad the 16 / 32-channel groups, fresh and accumulating destinations, the
    immediate and the deferred (table) reduction -- and against the direct form on the same operands."""
    import torch.nn.functional as F
    from reconvat_amd import ops, _lib
    lib = _lib.load()
    B = 3
    x = rnd(B, H, W, cin, seed=1).to(dev)
    dy = rnd(B, H, W, cout, seed=2).to(dev)
    wshape = (cout, cin, 3, 3) if kind == 'c3' else (cin, cout, 3, 3)
    w = rnd(*wshape, seed=3).to(dev)
    xt = x.cpu().permute(0, 3, 1, 2).double().requires_grad_(False)
    wt = w.cpu().double().requires_grad_(True)
    bt = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    yt = F.conv2d(xt, wt, bt, padding=1) if kind == 'c3' else F.conv_transpose2d(xt, wt, bt, padding=1)
    yt.backward(dy.cpu().permute(0, 3, 1, 2).double())
    old = ops.AUTOTUNE
    ops.AUTOTUNE = False                                    # (the plan is pinned by hand below)
    try:
        res = {}
        for name, nw in (('direct', 8), ('wino', 24)):
            assert lib.rv_conv_wgrad_set_plan(9, B, H, cin, cout, nw, 256) == 0
            dw, db = ops.conv_wgrad(kind, x, dy, w, True)
            res[name] = (dw.clone(), db.clone())
            # accumulate into existing gradients, immediate and deferred reduction
            for deferred in (False, True):
                gw, gb = torch.full_like(w, 0.5), torch.full((cout,), -0.25, device=dev)
                if deferred:
                    with ops.deferred_wgrad_reductions() as pend:
                        ops.conv_wgrad(kind, x, dy, w, True, gw, gb)
                        pend.flush()
                else:
                    ops.conv_wgrad(kind, x, dy, w, True, gw, gb)
                torch.cuda.synchronize()
                assert rel_err(gw - 0.5, dw) < 1e-5 and rel_err(gb + 0.25, db) < 1e-5, (name, deferred)
        assert rel_err(res['wino'][0], wt.grad.float()) < 2e-5, rel_err(res['wino'][0], wt.grad.float())
        assert rel_err(res['wino'][1], bt.grad.float()) < 2e-5
        assert rel_err(res['wino'][0], res['direct'][0]) < 2e-5
    finally:
        lib.rv_conv_wgrad_set_plan(9, B, H, cin, cout, 0, 0)
        ops.AUTOTUNE = old


def test_deterministic_mode_parameter_gradients(dev, monkeypatch):
    """RV_DETERMINISTIC=1 (ops.DETERMINISTIC): the parameter-gradient folds without fp32 atomics -- ordered column sums, ticketed in-order
    split-K with the bias row sums riding on it, per-layer weight-gradient reductions.  Repeated runs are bit-identical, and the values
    agree with the default (atomic) folds to rounding."""
    from reconvat_amd import ops, _lib
    x = torch.rand(5000, 229, device=dev) - 0.5
    out = torch.full((229,), 3.0, device=dev)
    ws = torch.empty(_lib.load().rv_colsum_ordered_workspace_bytes(5000, 229) // 4, device=dev)
    _lib.call('rv_colsum_ordered', x.data_ptr(), 229, 5000, 229, out.data_ptr(), 1, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rel_err(out - 3.0, x.double().sum(0).float()) < 1e-5
    # a strided narrow view over many rows (the up-conv bias gradient shape) -- accumulate = 0 overwrites
    y = torch.rand(300000, 24, device=dev)[:, :16]
    o2 = torch.full((16,), 9.0, device=dev)
    ws2 = torch.empty(_lib.load().rv_colsum_ordered_workspace_bytes(300000, 16) // 4, device=dev)
    _lib.call('rv_colsum_ordered', y.data_ptr(), 24, 300000, 16, o2.data_ptr(), 0, ws2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rel_err(o2, y.double().sum(0).float()) < 1e-5

    def grads(det):
        monkeypatch.setattr(ops, 'DETERMINISTIC', [det])
        torch.manual_seed(3)
        xin = (torch.rand(5120, 176, device=dev) - 0.5).requires_grad_(True)
        w = ((torch.rand(88, 176, device=dev) - 0.5) * 0.1).requires_grad_(True)
        b = torch.zeros(88, device=dev, requires_grad=True)
        yv = ops.LinearFn.apply(xin, w, b, 1)
        (yv * (torch.rand(5120, 88, device=dev) - 0.5)).sum().backward()
        cw = ((torch.rand(32, 16, 3, 3, device=dev) - 0.5) * 0.2).requires_grad_(True)
        cb = torch.zeros(32, device=dev, requires_grad=True)
        xi = torch.rand(2, 40, 57, 16, device=dev) - 0.5
        z = ops.ConvFn.apply(xi, cw, cb, 'c3', None)
        (z * (torch.rand_like(z) - 0.5)).sum().backward()
        return [t.grad.clone() for t in (xin, w, b, cw, cb)]
    d1, d2, a1 = grads(True), grads(True), grads(False)
    for p, q in zip(d1, d2):
        assert torch.equal(p, q)
    for p, q in zip(d1, a1):
        assert rel_err(p, q) < 1e-5


WGRAD_SEG_CASES = [('c3', 32, 32, 12, 57, 24), ('c3', 64, 64, 8, 28, 8), ('t3', 96, 48, 10, 57, 24), ('c3', 16, 16, 6, 229, 24), ('c1', 32, 64, 9, 57, 8),
                   ('down', 32, 32, 10, 57, 8), ('up', 32, 32, 5, 29, 8), ('c3', 48, 24, 7, 114, 8)]


@pytest.mark.parametrize('kind,cin,cout,H,W,nw', WGRAD_SEG_CASES)
@pytest.mark.parametrize('nseg', [2, 3, 4])
def test_wgrad_segments_equal_the_sum_of_per_pass_launches(dev, kind, cin, cout, H, W, nw, nseg):
    """rv_conv_wgrad_seg / rv_conv_wgrad_deferred_seg (ops.conv_wgrad_merged): ONE launch over the (x, dY) pairs of `nseg` backward passes of a
    layer adds the same dW / db into the gradient buffers as `nseg` separate launches (both against torch in fp64) -- Winograd and direct
    kernels, every conv kind with an MFMA weight-gradient kernel, odd heights, segments that live in unrelated allocations."""
    import torch.nn.functional as F
    from reconvat_amd import ops, _lib
    lib = _lib.load()
    B = 2
    ho, wo = ops._out_hw(kind, H, W, (2 * H + 1, 2 * W + 1) if kind == 'up' else None)
    wshape = {'c3': (cout, cin, 3, 3), 't3': (cin, cout, 3, 3), 'c1': (cout, cin, 1, 1), 'down': (cout, cin, 2, 2), 'up': (cin, cout, 2, 2)}[kind]
    w = rnd(*wshape, seed=3).to(dev)
    pairs, junk = [], []
    for sgi in range(nseg):
        junk.append(torch.empty(1000 + 4096 * sgi, device=dev))                   # (scatter the segments over the heap)
        pairs.append((rnd(B, H, W, cin, seed=10 + sgi).to(dev), rnd(B, ho, wo, cout, seed=20 + sgi).to(dev)))
    # torch: the sum over the passes of the layer's parameter gradients, fp64
    wt = w.cpu().double().requires_grad_(True)
    bt = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    for x, dy in pairs:
        xt = x.cpu().permute(0, 3, 1, 2).double()
        if kind == 'c3':
            yt = F.conv2d(xt, wt, bt, padding=1)
        elif kind == 't3':
            yt = F.conv_transpose2d(xt, wt, bt, padding=1)
        elif kind == 'c1':
            yt = F.conv2d(xt, wt, bt)
        elif kind == 'down':
            yt = F.conv2d(xt, wt, bt, stride=2)
        else:
            yt = F.conv_transpose2d(xt, wt, bt, stride=2, output_padding=(ho - 2 * H, wo - 2 * W))
        yt.backward(dy.cpu().permute(0, 3, 1, 2).double())
    taps = {'c3': 9, 't3': 9, 'c1': 1, 'down': 4, 'up': 4}[kind]
    hv, ca, cb = (H, cout, cin) if kind == 'up' else (ho, cin, cout)
    old = ops.AUTOTUNE
    ops.AUTOTUNE = False
    try:
        for bb in (B, nseg * B):
            assert lib.rv_conv_wgrad_set_plan(taps, bb, hv, ca, cb, nw, 256) == 0
        want_bias = kind != 'up'                                 # (the up-conv's bias gradient is a column sum of dY, taken per pass)
        for deferred in (False, True):
            gw, gb = torch.full_like(w, 0.5), torch.full((cout,), -0.25, device=dev)
            gw2, gb2 = gw.clone(), gb.clone()
            items = [(kind, x, dy, w, gw, gb if want_bias else None, False, torch.cuda.current_stream()) for x, dy in pairs]
            if deferred:
                with ops.deferred_wgrad_reductions() as pend:
                    assert ops.conv_wgrad_merged(items)
                    for x, dy in pairs:
                        ops.conv_wgrad(kind, x, dy, w, want_bias, gw2, gb2 if want_bias else None)
                    pend.flush()
            else:
                assert ops.conv_wgrad_merged(items)
                for x, dy in pairs:
                    ops.conv_wgrad(kind, x, dy, w, want_bias, gw2, gb2 if want_bias else None)
            torch.cuda.synchronize()
            assert rel_err(gw - 0.5, wt.grad.float()) < 3e-5, (deferred, rel_err(gw - 0.5, wt.grad.float()))
            assert rel_err(gw - 0.5, gw2 - 0.5) < 1e-5
            if want_bias:
                assert rel_err(gb + 0.25, bt.grad.float()) < 3e-5 and rel_err(gb + 0.25, gb2 + 0.25) < 1e-5
    finally:
        for bb in (B, nseg * B):
            lib.rv_conv_wgrad_set_plan(taps, bb, hv, ca, cb, 0, 0)
        ops.AUTOTUNE = old


def test_wgrad_merger_learns_then_merges(dev):
    """ops.WgradMerger: a step that runs unmerged teaches it how many passes add into a gradient buffer; from then on the passes only register
    and the last one launches -- same gradients, a third of the launches; a step that takes another path is finished by finish()."""
    from reconvat_amd import ops
    w = rnd(32, 32, 3, 3, seed=3).to(dev)
    pairs = [(rnd(2, 12, 57, 32, seed=10 + i).to(dev), rnd(2, 12, 57, 32, seed=20 + i).to(dev)) for i in range(3)]
    merger = ops.WgradMerger()
    launches = []
    hook_prev = ops._lib.HOOK[0]
    ops._lib.HOOK[0] = lambda name, args, fn: (launches.append(name), fn(*args))[1]
    try:
        results = []
        gw, gb = torch.zeros_like(w), torch.zeros(32, device=dev)           # (the merger knows a layer by its gradient buffer)
        for step, npass in enumerate((3, 3, 2, 3)):
            gw.zero_(), gb.zero_()
            launches.clear()
            with ops.wgrad_merging(merger, False):
                for x, dy in pairs[:npass]:
                    ops.conv_wgrad('c3', x, dy, w, True, gw, gb)
                merger.finish()
            torch.cuda.synchronize()
            results.append((gw.clone(), gb.clone(), [n for n in launches if n.startswith('rv_conv_wgrad')]))
    finally:
        ops._lib.HOOK[0] = hook_prev
    assert results[0][2] == ['rv_conv_wgrad'] * 3                                     # learning step: per pass
    assert results[1][2] == ['rv_conv_wgrad_seg']                                     # merged: one launch
    assert results[2][2] == ['rv_conv_wgrad_seg']                                     # a pass short: finish() launches the two that came
    assert results[3][2] == ['rv_conv_wgrad_seg', 'rv_conv_wgrad']                    # (learned 2 in the short step: the third pass arrives alone)
    assert rel_err(results[1][0], results[0][0]) < 1e-5 and rel_err(results[1][1], results[0][1]) < 1e-5
    assert rel_err(results[3][0], results[0][0]) < 1e-5


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('B,H,W,cin,C', [(2, 24, 57, 1, 16), (3, 12, 57, 16, 32), (2, 9, 28, 32, 64), (2, 10, 14, 64, 128),
                                         # the shipped shapes (B = 8: the plan table decides the separate launch's tile, incl. the K-split family)
                                         (8, 640, 229, 1, 16), (8, 320, 114, 16, 32), (8, 160, 57, 32, 64), (8, 80, 28, 64, 128)])
def test_bn_apply_with_fused_skip_equals_the_separate_skip_conv(dev, training, B, H, W, cin, C):
    """Round 6: an encoder block's `x12 += skip(x)` (model/UNet_onset.py:191,198; skip = 1x1 conv) evaluated INSIDE the BatchNorm apply kernel
    (rv_bn_lrelu_fwd_skip: a rank-1 fma for the single-channel block, an fmaf chain in the MFMA kernel's k order for 16 / 32 / 64 input channels -- plain or K-split
    form, whichever the separate launch would run) must be BIT-IDENTICAL to the conv launch + residual read it replaces: output, running statistics and every
    gradient (z, gamma, beta, x, skip weight, skip bias; the skip conv's own backward is launched from the fused node)."""
    from reconvat_amd import ops
    z0, x0 = rnd(B, H, W, C, seed=1), rnd(B, H, W, cin, seed=2)
    gam0, bet0 = rnd(C, seed=3) * 0.2 + 1.0, rnd(C, seed=4) * 0.1
    w0, b0 = rnd(C, cin, 1, 1, seed=5) * (1.0 / cin ** 0.5), rnd(C, seed=6)
    cot = rnd(B, H, W, C, seed=7).to(dev)
    assert ops.skip_conv_ksplit(x0.to(dev), C) is not None
    outs = []
    for fused in (False, True):
        z, x = z0.to(dev).requires_grad_(True), x0.to(dev).requires_grad_(True)
        gam, bet, w, b = (t.to(dev).clone().requires_grad_(True) for t in (gam0, bet0, w0, b0))
        rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), device=dev, dtype=torch.long)
        if fused:
            y = ops.BnActFn.apply(z, gam, bet, rm, rv, nbt, None, training, ops.SLOPE, None, None, x, w, b, None)
        else:
            sk = ops.ConvFn.apply(x, w, b, 'c1', None)
            y = ops.BnActFn.apply(z, gam, bet, rm, rv, nbt, sk, training, ops.SLOPE, None, None)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        outs.append([y.detach(), rm, rv, nbt, z.grad, gam.grad, bet.grad, x.grad, w.grad, b.grad])
    names = ['y', 'running_mean', 'running_var', 'num_batches_tracked', 'dz', 'dgamma', 'dbeta', 'dx', 'dw_skip', 'db_skip']
    for n, a, bb in zip(names, *outs):
        assert torch.equal(a, bb), (n, float((a.double() - bb.double()).abs().max()))
    if B * H * W > 100000:
        return
    # ... and against torch (the unfused path is covered elsewhere; this pins the fused one on its own)
    zt, xt = z0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C, momentum=0.1)
    bn.train(training)
    with torch.no_grad():
        bn.weight.copy_(gam0); bn.bias.copy_(bet0)
    yt = F.leaky_relu(bn(zt.permute(0, 3, 1, 2))) + F.conv2d(xt.permute(0, 3, 1, 2), w0, b0)          # NCHW views of the NHWC leaves
    (yt * cot.cpu().permute(0, 3, 1, 2)).sum().backward()
    assert rel_err(outs[1][0], yt.permute(0, 2, 3, 1)) < 1e-5
    assert rel_err(outs[1][4], zt.grad) < 1e-4 and rel_err(outs[1][7], xt.grad) < 1e-4
